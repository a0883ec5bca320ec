"""The streaming video statistics on the inputs where a float32 variance goes wrong: tests/_video_edge_cases.py (low variance,
one step, constant pixels, full swing, float32 out of range, a resumed state, a long stream), every case against float64 in
units of one rounding of a sample, with the bounds tests/test_video_edges_host.py measures on the CPU.

For every case ops.video_stats_batch along the schedule on planar frames is held to float64 and to the eager oracle.  The same
inputs then go through every other route, each held to the specification it already has, so that a value checked once is
checked everywhere: ops.video_stats_batches (one launch per call of up to 16 batches; (33, 31) through the per-batch
fallback), the interleaved layouts, and for uint8 / uint16 codes the ingest forms behind a black-level chain and behind a
data-dependent one (ops.video_stats_ingest_batch, ops.video_stats_ingest_batches), torch.equal to ops.ingest_transform +
ops.video_stats_batch, which in turn is held to the float64 statistics of the pixels the transform classes' own __call__
gives on the CPU.  Every figure in u goes, beside the reference's own and the bound, into the session's parity record
(_util.OBSERVED, labels "video edges <family> <route> mean | std"); profiles/video_edges_observed.json holds those records of
one run on the MI355X."""
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import _video_edge_cases as ve
from _util import OBSERVED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _record(family, route, k, err):
    """The worst error in u of one comparison against float64 (k = 0: mean, 1: std) into the session's parity record, beside
    what the float32 reference shows on the family and the bound; the routes that are not listed are bit-equal to one that is."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1].split("[")[0]
    OBSERVED.append({"test": test, "what": f"video edges {family} {route} {('mean', 'std')[k]}", "unit": "u",
                     "reference": ve.MEASURED[family][k], "norm": float(err.max()), "norm_tol": ve.BOUND[family][k],
                     "elem": float(err.max()), "elem_tol": ve.BOUND[family][k], "n": int(err.size)})


def linearize(x, lut, mode):
    from oracle import eager_torch as oe
    return x if mode is None else oe.icrf_forward(torch.from_numpy(x), torch.from_numpy(lut), mode).numpy()


def oracle(x, lut, mode, sched):
    from oracle import eager_torch as oe
    mean, std = oe.video_mean_std(torch.from_numpy(x), None if mode is None else torch.from_numpy(lut), mode, list(sched))
    return mean.numpy(), std.numpy()


def _same(a, b):
    """torch.equal, a NaN equal to a NaN (family E's non-finite pixels)."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _interleaved(stored, layout):
    """(N, C, H, W) planes -> (N, H, W, C) frames (BGR: what an OpenCV reader hands over)."""
    return np.ascontiguousarray((stored[:, ::-1] if layout == "nhwc_bgr" else stored).transpose(0, 2, 3, 1))


def _state(dev, case, mean0, m20):
    """An empty state is never read (NaN); family F's is given."""
    if mean0 is None:
        return [torch.full(case.shape, float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    return [torch.from_numpy(a).to(dev) for a in (mean0, m20)]


def _std(m2, n):
    """The std of the mean as compute_video_mean_and_std forms it from m2, in float32."""
    return (torch.sqrt(m2 * (1 / (n - 1))) / math.sqrt(n)).cpu().numpy()


def _check(case, route, mean, m2, x_lin, u, mean64, std64, mean_o, std_o, special, n):
    """mean and std within the family's bound of float64 and of the float32 reference, in u; E's marked pixels non-finite
    as the reference has them; no NaN anywhere else and no negative zero in the std."""
    got_mean, got_std = mean.cpu().numpy(), _std(m2, n)
    bound_m, bound_s = ve.BOUND[case.family]
    marked = np.zeros(case.shape, dtype=bool)
    for idx in special:
        marked[idx] = True
        assert np.isnan(got_mean[idx]) == np.isnan(mean_o[idx]) and not np.isfinite(got_mean[idx]), (case.name, route, idx, got_mean[idx])
        assert np.isnan(got_mean[idx]) or got_mean[idx] == mean_o[idx], (case.name, route, idx, got_mean[idx], mean_o[idx])
        assert np.isnan(got_std[idx]) == np.isnan(std_o[idx]) and not np.isfinite(got_std[idx]), (case.name, route, idx, got_std[idx])
    assert np.all(np.isfinite(got_mean[~marked])) and np.all(np.isfinite(got_std[~marked])), (case.name, route)
    assert not np.any(np.signbit(got_std[~marked])), (case.name, route, "negative std or -0.0")
    for k, (what, got, ref64, ref_o, bound) in enumerate((("mean", got_mean, mean64, mean_o, bound_m), ("std", got_std, std64, std_o, bound_s))):
        err = ve.errors_in_u(got, ref64, u)
        print(f"{case.name} {route} {what}: {err.max():.4g} u against float64 (bound {bound:.4g})")
        _record(case.family, route, k, err)
        assert err.max() <= bound, ve.describe_worst(err, x_lin, case, f"{route} {what} against float64")
        err_o = ve.errors_in_u(got, np.where(marked, np.nan, ref_o), u)
        assert err_o.max() <= bound, ve.describe_worst(err_o, x_lin, case, f"{route} {what} against the eager oracle")


def _walk(dev, case, frames, before, state, call):
    """One launch per batch along the schedule: call(frames of the batch, mean, m2, frames before it, batch index)."""
    mean, m2 = _state(dev, case, *state)
    k = 0
    for i, b in enumerate(case.sched):
        call(frames[k:k + b], mean, m2, before + k, i)
        k += b
    return mean, m2


def _grouped(dev, case, frames, before, state, call):
    """Calls of up to 16 batches: call(list of batches, mean, m2, frames before them, index of the first batch, one launch)."""
    mean, m2 = _state(dev, case, *state)
    i = 0
    for k, part in ve.chunks(case.sched):
        offs = np.concatenate([[0], np.cumsum(part)]) + k
        parts = [frames[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        call(parts, mean, m2, before + k, i, max(part) <= 32)
        i += len(part)
    return mean, m2


def _black_level(case, stored):
    """A black level below every level of the case (0 where the case holds code 0: C and D), and the range above it up to
    max_code."""
    black = (16.0 if case.dtype == "u16" else 4.0) if int(stored.min()) > 16 else 0.0
    return black, float(case.max_code) - black


@pytest.mark.parametrize("case", ve.CASES, ids=[c.name for c in ve.CASES])
def test_video_edges(dev, case):
    from clair_torch_amd import ops
    from clair_torch_amd.common import transforms as T
    r = ve.reference(case, linearize, oracle)
    inp, before = r.inp, r.inp.frames_before
    n = before + sum(case.sched)
    lut_d = None if case.mode is None else torch.from_numpy(r.lut).to(dev)
    kw = dict(lut=lut_d, interp=case.mode)
    max_code = None if case.dtype == "f32" else float(case.max_code)
    state = (r.mean0, r.m20)
    frames = torch.from_numpy(inp.stored).to(dev)

    # planar, one launch per batch: against float64 and the eager oracle
    mean, m2 = _walk(dev, case, frames, before, state,
                     lambda x, mean, m2, k, i: ops.video_stats_batch(x, mean, m2, k, max_code=max_code, **kw))
    _check(case, "planar", mean, m2, r.x_lin, r.u, r.mean64, r.std64, r.mean_o, r.std_o, inp.special, n)

    # several batches per call: the same bits
    mean_g, m2_g = _grouped(dev, case, frames, before, state, lambda parts, mean, m2, k, i, one: ops.video_stats_batches(
        parts, mean, m2, k, max_code=max_code, require_one_launch=one, **kw))
    assert _same(mean_g, mean) and _same(m2_g, m2), (case.name, "batches")

    # interleaved frames: the same bits
    for layout in ("nhwc", "nhwc_bgr"):
        il = torch.from_numpy(_interleaved(inp.stored, layout)).to(dev)
        mean_l, m2_l = _walk(dev, case, il, before, state,
                             lambda x, mean, m2, k, i: ops.video_stats_batch(x, mean, m2, k, max_code=max_code, layout=layout, **kw))
        assert _same(mean_l, mean) and _same(m2_l, m2), (case.name, layout)
    if case.dtype == "f32":
        return

    # the ingest forms: the same codes behind a black level, and behind a data-dependent Normalize of every batch
    black, span = _black_level(case, inp.stored)
    codes = torch.from_numpy(inp.stored.astype(np.float32))
    for chain in ("affine", "data"):
        data = chain == "data"
        stages = [("affine_data", 1.0, 0.0)] if data else [("affine", black, span, 1.0, 0.0)]
        # the pixels the transform classes' own __call__ gives on the CPU, batch by batch
        norm = T.Normalize() if data else T.Normalize(max_val=black + span, min_val=black)
        offs = np.concatenate([[0], np.cumsum(case.sched)])
        x = torch.cat([norm(codes[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]).numpy()
        assert x.dtype == np.float32
        lut, x_lin, u, mean64, std64, mean_o, std_o, mean0, m20 = ve.pixel_reference(case, x, linearize, oracle, before)
        st = (mean0, m20)
        consts = [ops.ingest_extrema(frames[int(a):int(b)], ops.data_stage_prefix(stages), "nchw") if data else None for a, b in zip(offs[:-1], offs[1:])]
        mean_p, m2_p = _walk(dev, case, frames, before, st, lambda x, mean, m2, k, i: ops.video_stats_batch(
            ops.ingest_transform(x, stages, consts=consts[i]), mean, m2, k, **kw))
        _check(case, f"ingest_{chain}", mean_p, m2_p, x_lin, u, mean64, std64, mean_o, std_o, {}, n)
        mean_f, m2_f = _walk(dev, case, frames, before, st, lambda x, mean, m2, k, i: ops.video_stats_ingest_batch(
            x, stages, mean, m2, k, consts=consts[i], **kw))
        assert torch.equal(mean_f, mean_p) and torch.equal(m2_f, m2_p), (case.name, chain, "ingest_batch")
        mean_b, m2_b = _grouped(dev, case, frames, before, st, lambda parts, mean, m2, k, i, one: ops.video_stats_ingest_batches(
            parts, stages, mean, m2, k, consts=consts[i:i + len(parts)] if data else None, require_one_launch=one, **kw))
        assert torch.equal(mean_b, mean_p) and torch.equal(m2_b, m2_p), (case.name, chain, "ingest_batches")


def _loader(frames, sched):
    from clair_torch_amd.datasets import StackDataset, custom_collate
    offs = np.concatenate([[0], np.cumsum(sched)])
    sampler = [list(range(int(a), int(b))) for a, b in zip(offs[:-1], offs[1:])]
    return DataLoader(StackDataset(frames, [1.0] * len(frames)), batch_sampler=sampler, collate_fn=custom_collate)


@pytest.mark.parametrize("per_launch", [1, 16])
def test_public_interface(dev, per_launch):
    """One family-A case (uint16, +-1 code, batches of 16, 17 and 31 frames) through compute_video_mean_and_std."""
    from clair_torch_amd.common import transforms as T
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.inference import compute_video_mean_and_std
    from clair_torch_amd.models import ICRFModelDirect
    case, = [c for c in ve.CASES if c.family == "A" and (c.dtype, c.max_code, c.arg, c.sched) == ("u16", 65535, 1, (16, 17, 31))]
    assert case.mode == "linear"
    r = ve.reference(case, linearize, oracle)
    model = ICRFModelDirect(icrf=torch.from_numpy(r.lut).clone(), interpolation_mode=InterpMode.LINEAR).to(dev)
    mean, std = compute_video_mean_and_std(_loader(torch.from_numpy(r.inp.stored), case.sched), "cuda", model,
                                           gpu_transforms=[T.CastTo("float32"), T.Normalize(65535, 0)], batches_per_launch=per_launch)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and tuple(mean.shape) == case.shape
    em, es = ve.worst_errors(r, mean.cpu().numpy(), std.cpu().numpy())
    _record("A", f"public_{per_launch}", 0, em), _record("A", f"public_{per_launch}", 1, es)
    assert em.max() <= ve.BOUND["A"][0], ve.describe_worst(em, r.x_lin, case, "public interface mean")
    assert es.max() <= ve.BOUND["A"][1], ve.describe_worst(es, r.x_lin, case, "public interface std")


@pytest.mark.parametrize("per_launch", [1, 16])
def test_constant_frames_behind_a_data_dependent_chain_raise(dev, per_launch):
    """Every pixel of every frame the same code: a data-dependent Normalize has a zero range -- the reference's ValueError,
    not a value."""
    from clair_torch_amd.common import transforms as T
    from clair_torch_amd.inference import compute_video_mean_and_std
    frames = torch.full((8, 3, 5, 7), 300, dtype=torch.int32).to(torch.uint16)
    with pytest.raises(ValueError, match="Normalization range is zero"):
        compute_video_mean_and_std(_loader(frames, (4, 4)), "cuda", None, gpu_transforms=[T.CastTo("float32"), T.Normalize()],
                                   batches_per_launch=per_launch)
