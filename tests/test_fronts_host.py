"""CPU tests: what every front of clair_torch_amd.ops beside the HDR merge hands to the library -- the 26 entry points from
ct_linearize_std to ct_video_stats_ingest_batches.  As in test_merge_fronts_host.py ``nv.load()`` is replaced by a recording object,
``ops._require_device``, ``ops._stream`` and ``torch.cuda.device`` are patched so that CPU tensors go through, and nothing is
launched.  The recorder serves any ``ct_*`` name: one ending in ``_workspace`` answers WORKSPACE_BYTES, every other records its
arguments and answers the scripted status.

Unlike the merge contract the record holds what stands behind every ``ctypes.byref(...)``: each field of the geometry and of the pair
parameters, the table's size, mode and the tensor it points to, and kind and constants of each stage handed over.  Pointers are named
after the tensor passed in ("buffer": memory the front made itself, None: NULL).  When an entry point is called, a live tensor
must own the memory behind every pointer it gets -- a copy a front made and dropped before the call is "freed", which the record
never holds.

``tests/golden/fronts_host.json`` was written by ``python tests/test_fronts_host.py`` from ops.py before its fronts were given one call
tail, one explicit-std prelude and shared halves -- it is the contract.  Per case: the calls made under status 0 with every argument;
shape, dtype and identity of what came back; and, for every call of that sequence, the error raised when that call answers
ERR_UNSUPPORTED after the ones in front answered 0 (NativeLibraryError naming that entry point).  A case that is refused where
tests/test_ops_refusals_host.py cannot hold it (at that commit behind ``nv.load()``, which that table forbids to reach; no entry
point recorded) holds the exception instead: among them the unknown ``std_mode`` of ``linearize_frames`` and ``dark_field_blur``, a
KeyError where every other front raises ValueError.  Since then the mode is looked up while the arguments of ``_call`` are built, in
front of ``nv.load()``; the exception is the same."""
import contextlib
import ctypes
import gc
import json
import os
import warnings
from types import SimpleNamespace

import pytest
import torch

from clair_torch_amd import _native as nv
from clair_torch_amd import ops

CPU = torch.device("cpu")
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fronts_host.json")
WORKSPACE_BYTES = 64
AFF, CLAMP, DATA = ("affine", 64.0, 1000.0, 1.0, 0.0), ("clamp", [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)]), ("affine_data", 1.0, 0.0)
ENTRY_POINTS = ("ct_linearize_std", "ct_linearize_fwd", "ct_linearize_bwd", "ct_linearize_dark", "ct_linearize_ingest",
                "ct_linearize_ingest_data", "ct_linearize_ingest_strided", "ct_linearize_dark_ingest", "ct_dark_field_blur",
                "ct_pair_residual_fwd", "ct_pair_residual_bwd", "ct_pair_residual_ingest_fwd", "ct_pair_residual_ingest_bwd",
                "ct_band_stats", "ct_flatfield_sums", "ct_flatfield_apply", "ct_strided_downscale", "ct_export_cv",
                "ct_ingest_transform", "ct_ingest_transform_data", "ct_ingest_extrema", "ct_ingest_extrema_frames",
                "ct_video_stats_batch", "ct_video_stats_batches", "ct_video_stats_ingest_batch", "ct_video_stats_ingest_batches")


class Library:
    """Stands for the loaded library: ``ct_*_workspace`` answers WORKSPACE_BYTES, every other ``ct_*`` records (name, arguments as
    plain values) and returns the next status of ``script`` (the last one again once the script is used up)."""

    def __init__(self, script, names, check_live=True):
        self.script, self.names, self.calls, self.check_live, self.live = list(script), names, [], check_live, []

    @staticmethod
    def ct_error_string(rc):
        return f"status {rc}".encode()

    def _name(self, address):
        if not address or address in self.names:
            return self.names.get(address)
        return "buffer" if not self.check_live or any(start <= address < end for start, end in self.live) else "freed"

    @staticmethod
    def _live_memory():
        """[start, end) of the storage of every tensor alive now."""
        spans = set()
        with warnings.catch_warnings():      # (isinstance touches every object alive, deprecated ones among them)
            warnings.simplefilter("ignore")
            for o in gc.get_objects():
                if isinstance(o, torch.Tensor) and o.device.type == "cpu":
                    storage = o.untyped_storage()
                    spans.add((storage.data_ptr(), storage.data_ptr() + storage.nbytes()))
        return spans

    def _struct(self, s):
        fields = {name: getattr(s, name) for name, _ in s._fields_}
        if isinstance(s, nv.Icrf):
            fields["lut_dev"] = self._name(s.lut_dev)
        if isinstance(s, nv.IngestStage):
            fields["lo"], fields["hi"] = list(s.lo), list(s.hi)
        return fields

    def _plain(self, a, following):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, ctypes.c_void_p):
            return self._name(a.value)
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
            return [self._name(v) for v in a]
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int32:
            return list(a)
        if isinstance(a, ctypes.Array) and a._type_ is nv.IngestStage:      # (the stage count follows the array in every entry point)
            return [self._struct(a[k]) for k in range(following)]
        return self._struct(a._obj)      # ctypes.byref(...)

    def __getattr__(self, entry):
        if not entry.startswith("ct_"):
            raise AttributeError(entry)
        if entry.endswith("_workspace"):
            return lambda *args: WORKSPACE_BYTES

        def call(*args):
            self.live = self._live_memory() if self.check_live else []
            # memory freed too early is soon handed out again: an address that two pointer arguments share and that is no input's
            # has no owner either (the later tensor took the place of the one the earlier pointer meant)
            unnamed = [a.value for a in args if isinstance(a, ctypes.c_void_p) and a.value and a.value not in self.names]
            self.live = [span for span in self.live if not any(unnamed.count(v) > 1 and span[0] <= v < span[1] for v in unnamed)]
            self.calls.append([entry, [self._plain(a, args[i + 1] if i + 1 < len(args) else None) for i, a in enumerate(args)]])
            return self.script.pop(0) if len(self.script) > 1 else self.script[0]
        return call


def _inputs():
    """Everything a front can take, on stacks of 2 x 3 x 4 x 6, and the names of the pointers."""
    def u16(*shape):
        return torch.zeros(shape, dtype=torch.uint16)

    def f32(*shape):
        return torch.zeros(shape, dtype=torch.float32)

    def f64(*shape):
        return torch.zeros(shape, dtype=torch.float64)

    t = dict(frames=u16(2, 3, 4, 6), pixels=f32(2, 3, 4, 6), bgr=u16(2, 4, 6, 3), apart=u16(2, 2, 3, 4, 6), one=u16(1, 3, 4, 6),
             batch1=u16(2, 3, 4, 6), batch2=u16(1, 3, 4, 6), bgr1=u16(2, 4, 6, 3), bgr2=u16(1, 4, 6, 3), nothing=u16(0, 3, 4, 6),
             std=f32(2, 3, 4, 6), std_bgr=f32(2, 4, 6, 3), std_small=f32(2, 3, 2, 3), std_one=f32(1, 3, 4, 6),
             std_turned=f32(2, 3, 6, 4).transpose(2, 3), std_turned_bgr=f32(2, 4, 3, 6).transpose(2, 3), std_f64=f64(2, 3, 4, 6),
             lin=f32(2, 3, 4, 6), lin_std=f32(2, 3, 4, 6), lin_small=f32(2, 3, 2, 3), lin_std_small=f32(2, 3, 2, 3),
             lin_one=f32(1, 3, 4, 6), lin_std_one=f32(1, 3, 4, 6), lin_nothing=f32(0, 3, 4, 6), lin_std_nothing=f32(0, 3, 4, 6),
             dark=f32(2, 3, 4, 6), dark_std=f32(2, 3, 4, 6), dark_a=f32(3, 4, 6), dark_std_a=f32(3, 4, 6), dark_b=f32(1, 3, 4, 6),
             dark_std_b=f32(1, 3, 4, 6), halo=u16(2, 3, 2, 6),
             consts=f32(4), consts1=f32(4), consts2=f32(4), frame_consts=f32(2, 4), workspace=f32(32),
             lut=torch.linspace(0.0, 1.0, 16).repeat(3, 1), lut_long=torch.linspace(0.0, 1.0, 64).repeat(3, 1), grad_out=f32(2, 3, 4, 6),
             center=f64(1, 3), smean=f64(1, 3), coef=f64(1, 3), no_coef=f64(0, 3),
             mean=f64(3, 4, 6), mean_std=f32(3, 4, 6), flat=f32(3, 4, 6), flat_std=f32(3, 4, 6), mean_state=f32(3, 4, 6),
             m2_state=f32(3, 4, 6), down=u16(2, 3, 2, 3), down_bgr=u16(2, 2, 3, 3), same=u16(2, 3, 4, 6),
             plane=f32(4, 6), cv=f64(2, 4, 6, 3), cv_image=f32(4, 6, 3), ingested=f32(2, 3, 4, 6))
    names = {v.data_ptr(): name for name, v in t.items() if v.numel()}
    assert len(names) == sum(1 for v in t.values() if v.numel())
    t["pairs"] = ops.PairList(torch.tensor([0]), torch.tensor([1]), torch.tensor([2.0]), 2, CPU)
    t["no_pairs"] = ops.PairList(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0), 2, CPU)
    for field in ("i", "j", "ratio", "part_off", "part_sample", "part_pair"):
        names[getattr(t["pairs"], field).data_ptr()] = f"pairs.{field}"
    return SimpleNamespace(**t), names


TILE = ops.TileGeometry(h_global=12, row_offset=4)
PAIR = dict(interp="linear", lower=0.05, upper=0.95, use_relative=True)
# every case: what is called, in the module ``ops`` under test, on the inputs ``t``
_CASES = {
    # ---- ct_linearize_std / _fwd / _bwd
    "linearize_frames/plain": lambda ops, t: ops.linearize_frames(t.frames, t.lut),
    "linearize_frames/pixels": lambda ops, t: ops.linearize_frames(t.pixels, t.lut, "catmull", std_mode="constant", std_value=0.01),
    "linearize_frames/interleaved": lambda ops, t: ops.linearize_frames(t.bgr, t.lut, layout="nhwc", std_mode="multiplier", std_value=0.5),
    "linearize_frames/rich": lambda ops, t: ops.linearize_frames(t.bgr, t.lut, "lookup", std=t.std_bgr, std_value=0.25, max_code=4095.0, tile=TILE,
                                                            layout="nhwc_bgr", out=(t.lin, t.lin_std)),
    "linearize_frames/rich_without_std": lambda ops, t: ops.linearize_frames(t.frames, t.lut, std=t.std, want_std=False, tile=TILE, out=(t.lin, None)),
    "linearize_frames/apart": lambda ops, t: ops.linearize_frames(t.apart[:, 0], t.lut),
    "linearize_frames/std_copied": lambda ops, t: ops.linearize_frames(t.frames, t.lut, std=t.std_turned),
    "linearize_frames/std_converted": lambda ops, t: ops.linearize_frames(t.bgr, t.lut, std=t.std_turned_bgr.double(), layout="nhwc"),
    "linearize_frames/std_mode": lambda ops, t: ops.linearize_frames(t.frames, t.lut, std_mode="foo"),
    "icrf_forward/plain": lambda ops, t: ops.icrf_forward(t.pixels, t.lut, "linear"),
    "icrf_forward/rich": lambda ops, t: ops.icrf_forward(t.pixels, t.lut, "catmull", tile=TILE),
    "icrf_backward/plain": lambda ops, t: ops.icrf_backward(t.pixels, t.grad_out, t.lut, "linear", True, True),
    "icrf_backward/image_only": lambda ops, t: ops.icrf_backward(t.pixels, t.grad_out, t.lut, "catmull", True, False, tile=TILE),
    "icrf_backward/lut_only": lambda ops, t: ops.icrf_backward(t.pixels, t.grad_out, t.lut, "linear", False, True),
    # ---- ct_linearize_dark
    "linearize_dark_frames/plain": lambda ops, t: ops.linearize_dark_frames(t.frames, t.dark, t.dark_std, t.lut),
    "linearize_dark_frames/rich": lambda ops, t: ops.linearize_dark_frames(t.frames, [t.dark_a, t.dark_b], [t.dark_std_a, t.dark_std_b], t.lut,
                                                                      "catmull", std=t.std, std_value=0.25, max_code=4095.0, threshold=0.1,
                                                                      alpha=20.0, out=(t.lin, t.lin_std)),
    "linearize_dark_frames/shared_dark": lambda ops, t: ops.linearize_dark_frames(t.pixels, [t.dark_a, t.dark_a], [t.dark_std_a, t.dark_std_a], t.lut,
                                                                             std_mode="constant", std_value=0.01),
    "linearize_dark_frames/apart": lambda ops, t: ops.linearize_dark_frames(t.apart[:, 0], t.dark, t.dark_std, t.lut, std_mode="multiplier",
                                                                       std_value=0.5),
    "linearize_dark_frames/std_copied": lambda ops, t: ops.linearize_dark_frames(t.apart[:, 0], t.dark, t.dark_std, t.lut, std=t.std_turned),
    "linearize_dark_frames/single_frame": lambda ops, t: ops.linearize_dark_frames(t.apart[:1, 0], [t.dark_a], [t.dark_std_a], t.lut,
                                                                              out=(t.lin_one, t.lin_std_one)),
    "linearize_dark_frames/single_frame_with_std": lambda ops, t: ops.linearize_dark_frames(t.apart[:1, 0], t.dark_b, t.dark_std_b, t.lut,
                                                                                       std=t.std_one),
    # ---- ct_linearize_ingest / _data / _strided
    "linearize_ingest_frames/plain": lambda ops, t: ops.linearize_ingest_frames(t.frames, [AFF], t.lut),
    "linearize_ingest_frames/pixels": lambda ops, t: ops.linearize_ingest_frames(t.pixels, [AFF, CLAMP], t.lut, "catmull", std_mode="constant",
                                                                            std_value=0.01),
    "linearize_ingest_frames/interleaved": lambda ops, t: ops.linearize_ingest_frames(t.bgr, [AFF], t.lut, layout="nhwc"),
    "linearize_ingest_frames/no_stages": lambda ops, t: ops.linearize_ingest_frames(t.frames, [], t.lut),
    "linearize_ingest_frames/rich": lambda ops, t: ops.linearize_ingest_frames(t.bgr, [AFF, DATA, CLAMP], t.lut, "lookup", std=t.std, std_value=0.25,
                                                                          tile=TILE, layout="nhwc_bgr", out=(t.lin, t.lin_std),
                                                                          consts=t.frame_consts),
    "linearize_ingest_frames/rich_without_std": lambda ops, t: ops.linearize_ingest_frames(t.frames, [AFF], t.lut, std=t.std, want_std=False,
                                                                                      out=(t.lin, None), consts=t.frame_consts),
    "linearize_ingest_frames/std_copied": lambda ops, t: ops.linearize_ingest_frames(t.bgr, [AFF], t.lut, std=t.std_turned, layout="nhwc"),
    "linearize_ingest_frames/empty": lambda ops, t: ops.linearize_ingest_frames(t.nothing, [AFF], t.lut),
    "linearize_ingest_frames/empty_out": lambda ops, t: ops.linearize_ingest_frames(t.nothing, [AFF], t.lut, out=(t.lin_nothing, t.lin_std_nothing)),
    "linearize_ingest_frames_strided/plain": lambda ops, t: ops.linearize_ingest_frames_strided(t.frames, 2, [AFF], t.lut),
    "linearize_ingest_frames_strided/step_1": lambda ops, t: ops.linearize_ingest_frames_strided(t.frames, 1, [AFF], t.lut, tile=TILE),
    "linearize_ingest_frames_strided/pixels": lambda ops, t: ops.linearize_ingest_frames_strided(t.pixels, 2, [AFF, CLAMP], t.lut, "catmull",
                                                                                                 std_mode="constant", std_value=0.01),
    "linearize_ingest_frames_strided/interleaved": lambda ops, t: ops.linearize_ingest_frames_strided(t.bgr, 3, [AFF], t.lut, layout="nhwc"),
    "linearize_ingest_frames_strided/rich": lambda ops, t: ops.linearize_ingest_frames_strided(
        t.bgr, 2, [AFF, DATA], t.lut, "catmull", std=t.std_small, std_value=0.25, layout="nhwc_bgr", out=(t.lin_small, t.lin_std_small),
        consts=t.frame_consts),
    "linearize_ingest_frames_strided/rich_without_std": lambda ops, t: ops.linearize_ingest_frames_strided(
        t.frames, 2, [AFF], t.lut, std_mode="multiplier", std_value=0.5, want_std=False, out=(t.lin_small, None)),
    "linearize_ingest_frames_strided/empty": lambda ops, t: ops.linearize_ingest_frames_strided(t.nothing, 2, [AFF], t.lut),
    "linearize_ingest_frames_strided/step_bool": lambda ops, t: ops.linearize_ingest_frames_strided(t.frames, True, [AFF], t.lut),
    # ---- ct_linearize_dark_ingest
    "linearize_dark_ingest_frames/plain": lambda ops, t: ops.linearize_dark_ingest_frames(t.frames, [AFF], t.dark, t.dark_std, t.lut),
    "linearize_dark_ingest_frames/pixels": lambda ops, t: ops.linearize_dark_ingest_frames(t.pixels, [AFF, CLAMP], t.dark, t.dark_std, t.lut,
                                                                                           "catmull", std_mode="multiplier", std_value=0.5),
    "linearize_dark_ingest_frames/std_copied": lambda ops, t: ops.linearize_dark_ingest_frames(t.frames, [AFF], t.dark, t.dark_std, t.lut,
                                                                                               std=t.std_turned),
    "linearize_dark_ingest_frames/interleaved": lambda ops, t: ops.linearize_dark_ingest_frames(t.bgr, [AFF], t.dark, t.dark_std, t.lut, layout="nhwc",
                                                                                           std_mode="constant", std_value=0.01),
    "linearize_dark_ingest_frames/rich": lambda ops, t: ops.linearize_dark_ingest_frames(
        t.bgr, [AFF, CLAMP], [t.dark_a, t.dark_b], [t.dark_std_a, t.dark_std_b], t.lut, "catmull", std=t.std, std_value=0.25, layout="nhwc_bgr",
        out=(t.lin, t.lin_std), threshold=0.1, alpha=20.0),
    "linearize_dark_ingest_frames/single_frame": lambda ops, t: ops.linearize_dark_ingest_frames(t.one, [AFF], [t.dark_a], [t.dark_std_a], t.lut,
                                                                                            out=(t.lin_one, t.lin_std_one)),
    # ---- ct_dark_field_blur
    "dark_field_blur/plain": lambda ops, t: ops.dark_field_blur(t.frames, t.dark, None),
    "dark_field_blur/pixels": lambda ops, t: ops.dark_field_blur(t.pixels, t.dark_b, None, std_mode="constant", std_value=0.01),
    "dark_field_blur/rich": lambda ops, t: ops.dark_field_blur(t.frames, t.dark, t.dark_std, std=t.std, std_value=0.25, max_code=4095.0, tile=TILE,
                                                          halo=t.halo, threshold=0.1, alpha=20.0),
    "dark_field_blur/std_copied": lambda ops, t: ops.dark_field_blur(t.pixels, t.dark, t.dark_std, std=t.std_turned),
    "dark_field_blur/std_mode": lambda ops, t: ops.dark_field_blur(t.frames, t.dark, None, std_mode="foo"),
    # ---- ct_pair_residual_fwd / _bwd
    "pair_residual_sums/plain": lambda ops, t: ops.pair_residual_sums(t.frames, t.pairs, lut=t.lut, use_unc_weight=False, **PAIR),
    "pair_residual_sums/pixels": lambda ops, t: ops.pair_residual_sums(t.pixels, t.pairs, lut=None, use_unc_weight=True, std_mode="constant",
                                                                  std_value=0.01, **dict(PAIR, interp=None, use_relative=False)),
    "pair_residual_sums/rich": lambda ops, t: ops.pair_residual_sums(t.bgr, t.pairs, lut=t.lut, use_unc_weight=True, std=t.std_bgr, std_value=0.25,
                                                                max_code=4095.0, level=2, tile=TILE, center=t.center, layout="nhwc_bgr", **PAIR),
    "pair_residual_sums/std_copied": lambda ops, t: ops.pair_residual_sums(t.frames, t.pairs, lut=t.lut, use_unc_weight=True, std=t.std_turned,
                                                                           center=t.center.float(), **PAIR),
    "pair_residual_sums/no_pairs": lambda ops, t: ops.pair_residual_sums(t.frames, t.no_pairs, lut=t.lut, use_unc_weight=False, **PAIR),
    "pair_residual_lut_grad/plain": lambda ops, t: ops.pair_residual_lut_grad(t.frames, t.pairs, t.coef, lut=t.lut, **PAIR),
    "pair_residual_lut_grad/std_dropped": lambda ops, t: ops.pair_residual_lut_grad(t.frames, t.pairs, t.coef, lut=t.lut, std=t.std, std_mode="foo",
                                                                               smean=t.smean, **PAIR),
    "pair_residual_lut_grad/rich": lambda ops, t: ops.pair_residual_lut_grad(t.bgr, t.pairs, t.coef, lut=t.lut, max_code=4095.0, tile=TILE,
                                                                        use_unc_weight=True, std=t.std_bgr, std_value=0.25, smean=t.smean,
                                                                        lane_kernel=False, layout="nhwc_bgr", **PAIR),
    "pair_residual_lut_grad/weighted_constant": lambda ops, t: ops.pair_residual_lut_grad(t.pixels, t.pairs, t.coef, lut=t.lut, use_unc_weight=True,
                                                                                     std_mode="constant", std_value=0.01, smean=t.smean, **PAIR),
    "pair_residual_lut_grad/std_copied": lambda ops, t: ops.pair_residual_lut_grad(t.frames, t.pairs, t.coef.float(), lut=t.lut,
                                                                                   use_unc_weight=True, std=t.std_f64, smean=t.smean.float(),
                                                                                   **PAIR),
    "pair_residual_lut_grad/no_pairs": lambda ops, t: ops.pair_residual_lut_grad(t.frames, t.no_pairs, t.no_coef, lut=t.lut, **PAIR),
    # ---- ct_pair_residual_ingest_fwd / _bwd
    "pair_residual_ingest_sums/plain": lambda ops, t: ops.pair_residual_ingest_sums(t.frames, [AFF], t.pairs, lut=t.lut, use_unc_weight=False, **PAIR),
    "pair_residual_ingest_sums/rich": lambda ops, t: ops.pair_residual_ingest_sums(t.bgr, [AFF, DATA], t.pairs, lut=t.lut, use_unc_weight=True,
                                                                              consts=t.consts, std=t.std, std_value=0.25, level=2, tile=TILE,
                                                                              center=t.center, layout="nhwc_bgr", **PAIR),
    "pair_residual_ingest_sums/std_copied": lambda ops, t: ops.pair_residual_ingest_sums(t.frames, [AFF], t.pairs, lut=t.lut, use_unc_weight=True,
                                                                                         std=t.std_turned, center=t.center.float(), **PAIR),
    "pair_residual_ingest_sums/no_pairs": lambda ops, t: ops.pair_residual_ingest_sums(t.frames, [AFF], t.no_pairs, lut=t.lut, use_unc_weight=False,
                                                                                  **PAIR),
    "pair_residual_ingest_lut_grad/plain": lambda ops, t: ops.pair_residual_ingest_lut_grad(t.frames, [AFF], t.pairs, t.coef, lut=t.lut, **PAIR),
    "pair_residual_ingest_lut_grad/std_dropped": lambda ops, t: ops.pair_residual_ingest_lut_grad(t.frames, [AFF], t.pairs, t.coef, lut=t.lut, std=t.std,
                                                                                             std_mode="foo", smean=t.smean, **PAIR),
    "pair_residual_ingest_lut_grad/rich": lambda ops, t: ops.pair_residual_ingest_lut_grad(
        t.bgr, [AFF, DATA], t.pairs, t.coef, lut=t.lut, consts=t.consts, tile=TILE, use_unc_weight=True, std=t.std, std_value=0.25,
        smean=t.smean, lane_kernel=False, layout="nhwc_bgr", **PAIR),
    "pair_residual_ingest_lut_grad/std_copied": lambda ops, t: ops.pair_residual_ingest_lut_grad(
        t.bgr, [AFF], t.pairs, t.coef, lut=t.lut_long, use_unc_weight=True, std=t.std_turned, smean=t.smean, layout="nhwc", **PAIR),
    # (nothing the backward half allocates fits where a dropped copy of the std stood: the gradient of a 64-point table is larger)
    "pair_residual_ingest_lut_grad/no_pairs": lambda ops, t: ops.pair_residual_ingest_lut_grad(t.frames, [AFF], t.no_pairs, t.no_coef, lut=t.lut,
                                                                                          **PAIR),
    # ---- ct_band_stats, ct_flatfield_sums / _apply
    "band_stats/plain": lambda ops, t: ops.band_stats(t.mean),
    "band_stats/rich": lambda ops, t: ops.band_stats(t.mean, t.mean_std),
    "flatfield_correct/merged_mean": lambda ops, t: ops.flatfield_correct(t.mean, t.mean_std, t.flat, t.flat_std, input_is_variance=True,
                                                                     through_mean=True),
    "flatfield_correct/frames": lambda ops, t: ops.flatfield_correct(t.lin, t.lin_std, t.flat, None, input_is_variance=False, through_mean=False),
    "flatfield_correct/rich": lambda ops, t: ops.flatfield_correct(t.mean, None, t.flat, t.flat_std, input_is_variance=False, through_mean=True,
                                                              global_pixels=72, reduce=lambda sums: None),
    # ---- ct_strided_downscale, ct_export_cv
    "strided_downscale/plain": lambda ops, t: ops.strided_downscale(t.frames, 2),
    "strided_downscale/pixels": lambda ops, t: ops.strided_downscale(t.pixels, 3),
    "strided_downscale/rich": lambda ops, t: ops.strided_downscale(t.bgr, 2, layout="nhwc_bgr", out=t.down_bgr),
    "strided_downscale/out": lambda ops, t: ops.strided_downscale(t.frames, 2, out=t.down),
    "strided_downscale/step_1": lambda ops, t: ops.strided_downscale(t.frames, 1),
    "strided_downscale/step_1_out": lambda ops, t: ops.strided_downscale(t.frames, 1, out=t.same),
    "strided_downscale/empty": lambda ops, t: ops.strided_downscale(t.nothing, 2),
    "export_cv/plane": lambda ops, t: ops.export_cv(t.plane),
    "export_cv/image": lambda ops, t: ops.export_cv(t.mean),
    "export_cv/frames": lambda ops, t: ops.export_cv(t.lin, torch.float64),
    "export_cv/rich": lambda ops, t: ops.export_cv(t.lin, torch.float64, out=t.cv),
    "export_cv/image_out": lambda ops, t: ops.export_cv(t.mean, torch.float32, out=t.cv_image),
    "export_cv/empty": lambda ops, t: ops.export_cv(t.lin_nothing),
    # ---- ct_ingest_transform / _data, ct_ingest_extrema / _frames
    "ingest_transform/plain": lambda ops, t: ops.ingest_transform(t.frames, [AFF]),
    "ingest_transform/pixels": lambda ops, t: ops.ingest_transform(t.pixels, [AFF, CLAMP]),
    "ingest_transform/interleaved": lambda ops, t: ops.ingest_transform(t.bgr, [AFF], "nhwc"),
    "ingest_transform/rich": lambda ops, t: ops.ingest_transform(t.bgr, [AFF, DATA, CLAMP], "nhwc_bgr", out=t.ingested, consts=t.consts),
    "ingest_transform/consts_without_data_stage": lambda ops, t: ops.ingest_transform(t.frames, [AFF], consts=t.consts),
    "ingest_transform/empty": lambda ops, t: ops.ingest_transform(t.nothing, [AFF]),
    "ingest_transform/empty_out": lambda ops, t: ops.ingest_transform(t.nothing, [AFF], out=t.lin_nothing, consts=t.consts),
    "ingest_transform_data/plain": lambda ops, t: ops.ingest_transform_data(t.frames, [AFF, DATA], check=False),
    "ingest_transform_data/pixels": lambda ops, t: ops.ingest_transform_data(t.pixels, [DATA, CLAMP], max_val=1.0, check=False),
    "ingest_transform_data/rich": lambda ops, t: ops.ingest_transform_data(t.bgr, [AFF, DATA, CLAMP], "nhwc_bgr", min_val=0.5, check=False,
                                                                      out=t.ingested),
    "ingest_extrema/plain": lambda ops, t: ops.ingest_extrema(t.frames),
    "ingest_extrema/rich": lambda ops, t: ops.ingest_extrema(t.bgr, [AFF, CLAMP], "nhwc_bgr", max_val=2.5),
    "ingest_extrema/fixed_min": lambda ops, t: ops.ingest_extrema(t.pixels, [AFF], min_val=1),
    "ingest_extrema_frames/plain": lambda ops, t: ops.ingest_extrema_frames(t.frames),
    "ingest_extrema_frames/rich": lambda ops, t: ops.ingest_extrema_frames(t.bgr, [AFF, CLAMP], "nhwc_bgr", None, 2.5, out=t.frame_consts,
                                                                      workspace=t.workspace),
    "ingest_extrema_frames/fixed_min": lambda ops, t: ops.ingest_extrema_frames(t.pixels, [AFF], min_val=1, out=t.frame_consts),
    "ingest_extrema_frames/workspace_only": lambda ops, t: ops.ingest_extrema_frames(t.frames, workspace=t.workspace),
    "ingest_extrema_frames/workspace_too_small": lambda ops, t: ops.ingest_extrema_frames(t.frames, workspace=t.workspace[:15]),
    "ingest_extrema_frames/out_shape": lambda ops, t: ops.ingest_extrema_frames(t.frames, out=t.consts),
    "ingest_extrema_frames_workspace/plain": lambda ops, t: ops.ingest_extrema_frames_workspace(3, CPU),
    # ---- ct_video_stats_batch / _batches / _ingest_batch / _ingest_batches
    "video_stats_batch/plain": lambda ops, t: ops.video_stats_batch(t.frames, t.mean_state, t.m2_state, 0),
    "video_stats_batch/rich": lambda ops, t: ops.video_stats_batch(t.bgr, t.mean_state, t.m2_state, 7, lut=t.lut, interp="catmull", max_code=4095.0,
                                                              tile=TILE, layout="nhwc_bgr"),
    "video_stats_batch/pixels": lambda ops, t: ops.video_stats_batch(t.pixels, t.mean_state, t.m2_state, 3, lut=t.lut, interp="linear"),
    "video_stats_batch/apart": lambda ops, t: ops.video_stats_batch(t.apart[:, 0], t.mean_state, t.m2_state, 2),
    "video_stats_batches/one_batch": lambda ops, t: ops.video_stats_batches([t.frames], t.mean_state, t.m2_state, 0),
    "video_stats_batches/one_batch_of_one_frame": lambda ops, t: ops.video_stats_batches([t.apart[:1, 0]], t.mean_state, t.m2_state, 0),
    "video_stats_batches/three_batches": lambda ops, t: ops.video_stats_batches([t.frames, t.batch1, t.batch2], t.mean_state, t.m2_state, 0),
    "video_stats_batches/pixels": lambda ops, t: ops.video_stats_batches([t.pixels, t.lin, t.lin_one], t.mean_state, t.m2_state, 3, lut=t.lut,
                                                                         interp="catmull"),
    "video_stats_batches/rich": lambda ops, t: ops.video_stats_batches([t.bgr, t.bgr1, t.bgr2], t.mean_state, t.m2_state, 7, lut=t.lut,
                                                                  interp="linear", max_code=4095.0, tile=TILE, layout="nhwc_bgr",
                                                                  require_one_launch=True),
    "video_stats_ingest_batch/plain": lambda ops, t: ops.video_stats_ingest_batch(t.frames, [AFF], t.mean_state, t.m2_state, 0),
    "video_stats_ingest_batch/rich": lambda ops, t: ops.video_stats_ingest_batch(t.bgr, [AFF, DATA, CLAMP], t.mean_state, t.m2_state, 7, lut=t.lut,
                                                                            interp="catmull", tile=TILE, layout="nhwc_bgr", consts=t.consts),
    "video_stats_ingest_batches/one_batch": lambda ops, t: ops.video_stats_ingest_batches([t.frames], [AFF], t.mean_state, t.m2_state, 0),
    "video_stats_ingest_batches/three_batches": lambda ops, t: ops.video_stats_ingest_batches([t.frames, t.batch1, t.batch2], [AFF], t.mean_state,
                                                                                         t.m2_state, 0),
    "video_stats_ingest_batches/rich": lambda ops, t: ops.video_stats_ingest_batches(
        [t.bgr, t.bgr1, t.bgr2], [AFF, DATA, CLAMP], t.mean_state, t.m2_state, 7, lut=t.lut, interp="linear", tile=TILE, layout="nhwc_bgr",
        consts=[t.consts, t.consts1, t.consts2], require_one_launch=True),
    "video_stats_ingest_batches/some_consts": lambda ops, t: ops.video_stats_ingest_batches([t.frames, t.batch1, t.batch2], [AFF, DATA], t.mean_state,
                                                                                       t.m2_state, 0, consts=[t.consts, None, t.consts2]),
    "video_stats_ingest_batches/one_batch_with_consts": lambda ops, t: ops.video_stats_ingest_batches([t.frames], [DATA], t.mean_state, t.m2_state, 0,
                                                                                                 consts=[t.consts]),
}
# the cases that must reach no entry point (status 0): the launch-skipping ones and those refused behind ``nv.load()``
NO_LAUNCH = ("linearize_frames/std_mode", "dark_field_blur/std_mode", "linearize_ingest_frames/empty", "linearize_ingest_frames/empty_out",
             "linearize_ingest_frames_strided/empty", "linearize_ingest_frames_strided/step_bool", "pair_residual_sums/no_pairs",
             "pair_residual_lut_grad/no_pairs", "pair_residual_ingest_sums/no_pairs", "pair_residual_ingest_lut_grad/no_pairs",
             "strided_downscale/step_1", "strided_downscale/step_1_out", "strided_downscale/empty", "export_cv/empty", "ingest_transform/empty",
             "ingest_transform/empty_out", "ingest_extrema_frames/workspace_too_small", "ingest_extrema_frames/out_shape",
             "ingest_extrema_frames_workspace/plain")


def _came_back(out, t):
    """Shape, dtype and identity (the name of the caller's tensor it IS, else None) of every tensor that came back."""
    if isinstance(out, tuple):
        return [_came_back(v, t) for v in out]
    if out is None:
        return None
    mine = [name for name, v in vars(t).items() if v is out]
    return dict(shape=list(out.shape), dtype=str(out.dtype), is_input=mine[0] if mine else None)


def _run(case, script, monkeypatch, check_live=True):
    """-> (the recorded calls, what came back | the exception as text)."""
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    t, names = _inputs()
    lib = Library(script, names, check_live)
    monkeypatch.setattr(ops.nv, "load", lambda: lib)
    try:
        back = _came_back(_CASES[case](ops, t), t)
    except Exception as e:    # noqa: BLE001 -- the type and the message are what is recorded
        back = f"{type(e).__name__}: {e}"
    return lib.calls, back


def _observe(case, monkeypatch):
    calls, back = _run(case, [0], monkeypatch)
    errors = []
    for k, (entry, _) in enumerate(calls):      # call k answers ERR_UNSUPPORTED, the ones in front of it 0
        failed, raised = _run(case, [0] * k + [nv.ERR_UNSUPPORTED], monkeypatch, check_live=False)
        assert failed == calls[:k + 1], f"{case}: the calls up to the failing {entry} differ from those of the run that passed"
        errors.append(raised)
    return json.loads(json.dumps(dict(calls=calls, back=back, errors=errors)))


_RECORDED = {}
if os.path.exists(RECORD):
    with open(RECORD) as _fh:
        _RECORDED = json.load(_fh)


def test_every_case_and_entry_point_is_recorded():
    assert set(_RECORDED) == set(_CASES)
    reached = {entry for rec in _RECORDED.values() for entry, _ in rec["calls"]}
    assert reached == set(ENTRY_POINTS)
    for case, rec in _RECORDED.items():
        assert (not rec["calls"]) == (case in NO_LAUNCH), case
        assert "AssertionError" not in str(rec["back"]) and '"freed"' not in json.dumps(rec["calls"])
        # a failing call raises NativeLibraryError naming its own entry point
        assert rec["errors"] == [f"NativeLibraryError: {entry}: status {nv.ERR_UNSUPPORTED} (code {nv.ERR_UNSUPPORTED})" for entry, _ in rec["calls"]]
    # the one difference a shared std prelude has to keep: these two look the mode up unchecked
    for case in ("linearize_frames/std_mode", "dark_field_blur/std_mode"):
        assert _RECORDED[case]["back"] == "KeyError: 'foo'"


@pytest.mark.parametrize("case", list(_CASES))
def test_calls_arguments_and_results(case, monkeypatch):
    assert _observe(case, monkeypatch) == _RECORDED[case]


if __name__ == "__main__":      # writes the record from the ops.py at hand
    with pytest.MonkeyPatch.context() as mp:
        record = {case: _observe(case, mp) for case in _CASES}
    with open(RECORD, "w") as fh:
        json.dump(record, fh, indent=0, sort_keys=True)
        fh.write("\n")
