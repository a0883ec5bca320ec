"""Seeded inputs of the pair-ingest tests (ct_pair_residual_ingest_fwd / _bwd, csrc/ct_pairs_ingest.hip): raw uint8 / uint16
scenes of tests/_pair_refs.py behind gpu_transforms chains, the chains evaluated on the CPU with the transform classes of
common/transforms.py (the reference's float32 arithmetic, which ct_ingest_transform reproduces bit for bit), and the float64
reference of _pair_refs on that chain output.  tests/test_pairs_ingest_host.py checks on the CPU that no chain masks its
scene away; tests/test_gpu_pairs_ingest.py compares the kernels.  Nothing here calls the code under test."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import _pair_refs as pr

TOP = {"u8": 255.0, "u16": 65535.0}
PLANES = pr.PLANES            # 13x17 odd plane, scalar stager; 12x20 vector stager, partial last tile; 8x64 whole tiles
LAYOUTS = ("nchw", "nhwc", "nhwc_bgr")
CHAINS = ("black", "range", "clamp", "clamp_channels", "four", "data")


def transforms_of(chain, dtype):
    """The gpu_transforms list of a named chain for codes of ``dtype`` (behind the CvToTorch that an interleaved BGR source
    adds in front).  Black levels and clamps are chosen so that most of the scene stays inside the validity thresholds."""
    from clair_torch_amd.common import transforms as T
    top = TOP[dtype]
    black = 4.0 if dtype == "u8" else 1024.0
    cast = T.CastTo("float32")
    if chain == "black":            # a black level: Normalize(max, min > 0)
        return [cast, T.Normalize(top, black)]
    if chain == "range":            # a target range
        return [cast, T.Normalize(top, 0.0, target_range=(0.02, 0.9))]
    if chain == "clamp":            # one clamp pair for every element
        return [cast, T.Normalize(top, 0.0), T.ClampAlongDims(1, (0.05, 0.9))]
    if chain == "clamp_channels":   # one pair per channel: the clamp pair is chosen by the plane's channel
        return [cast, T.Normalize(top, 0.0), T.ClampAlongDims(1, [(0.02, 0.95), (0.05, 0.9), (0.0, 0.8)])]
    if chain == "four":             # four stages: black level, clamp, target range, per-channel clamp
        return [cast, T.Normalize(top, black), T.ClampAlongDims(1, (0.0, 0.97)), T.Normalize(1.0, 0.0, target_range=(0.01, 0.99)),
                T.ClampAlongDims(1, [(0.01, 0.95), (0.03, 0.99), (0.01, 0.9)])]
    if chain == "data":             # one data-dependent Normalize: the batch's own extrema
        return [cast, T.Normalize()]
    raise KeyError(chain)


def chain_output(codes, chain, dtype):
    """The chain on planar (N, C, H, W) codes, on the CPU: float32 pixels."""
    x = codes
    for t in transforms_of(chain, dtype):
        x = t(x)
    return x.contiguous()


def stages_of(codes, chain, dtype):
    """(stages as ops.ingest_transform takes them, is the chain data-dependent) through plan_staging, as stage_images does."""
    from clair_torch_amd.common.transforms import plan_staging
    plan = plan_staging(codes, transforms_of(chain, dtype), on_device=True)
    assert plan.route == ("ingest_data" if chain == "data" else "ingest"), (chain, plan.route)
    return plan.stages, plan.route == "ingest_data"


def to_layout(t, layout):
    """Planar (N, C, H, W) RGB -> the memory order of ``layout`` (uint16 has no flip kernel: through int32)."""
    if layout == "nchw":
        return t.contiguous()
    if layout == "nhwc_bgr":
        wide = t.to(torch.int32) if t.dtype in (torch.uint8, torch.uint16) else t
        t = wide.flip(1).to(t.dtype)
    return t.permute(0, 2, 3, 1).contiguous()


def _repair(codes, chain, dtype, exposures, lut, interp, threshold):
    """pr.repair for a scene behind a chain: every valid pair sample whose residual is closer to zero than
    pr.RESIDUAL_BOUND (its sign would differ between two float32 orders) moves by one code, until none is left."""
    codes = codes.clone()
    for _ in range(8):
        x = chain_output(codes, chain, dtype)
        ref = pr.pair_step_f64(x, None, exposures, lut, interp, threshold, want_grad=False)
        bad = ref.valid & (ref.resid < pr.RESIDUAL_BOUND)
        if not bad.any():
            return codes, x
        p, cc, hh, ww = torch.nonzero(bad, as_tuple=True)
        a = codes.numpy()
        a[ref.i[p].numpy(), cc.numpy(), hh.numpy(), ww.numpy()] += 1
    raise AssertionError("repair did not converge")


@functools.lru_cache(maxsize=None)
def build(chain, dtype, plane, interp="linear"):
    """Namespace of a case: codes (planar (N, 3, H, W) uint8 / uint16), x (the chain's float32 output), chain, dtype,
    exposures, threshold, lut, interp, lo, hi, seed.  The repair is done for ``interp`` (the curve decides the residuals)."""
    seed = 5000 + 1000 * CHAINS.index(chain) + 7 * plane[0] + plane[1] + 500 * (dtype == "u16")
    cs = SimpleNamespace(name=f"{chain}_{dtype}_{plane[0]}x{plane[1]}_{interp}", chain=chain, dtype=dtype, plane=plane,
                         exposures=pr.base_exposures(), threshold=0.25, lut=pr.base_lut(), interp=interp, lo=pr.LO, hi=pr.HI,
                         seed=seed, h_global=None, row_offset=0)
    codes, _, _ = pr.scene(seed, cs.exposures, (3,) + tuple(plane), dtype)
    cs.codes, cs.x = _repair(codes, chain, dtype, cs.exposures, cs.lut if interp else None, interp, cs.threshold)
    return cs


def reference(cs, rel, unc=False, sd=None, want_grad=True, **kw):
    n_pairs = pr.exposure_pairs(cs.exposures, cs.threshold)[0].numel()
    return pr.pair_step_f64(cs.x, sd, cs.exposures, cs.lut if cs.interp else None, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc,
                            coef=pr.seeded_coef(cs, n_pairs), h_global=cs.h_global, row_offset=cs.row_offset,
                            want_grad=want_grad and cs.interp is not None, **kw)


def band_of(cs, r0, rows):
    """Rows [r0, r0 + rows) of a case with the global geometry attached (x is the chain output of the WHOLE image: a
    data-dependent chain keeps the whole image's extrema)."""
    out = SimpleNamespace(**vars(cs))
    out.name = f"{cs.name}_band{r0}+{rows}"
    out.codes, out.x = (t[:, :, r0:r0 + rows].contiguous() for t in (cs.codes, cs.x))
    out.h_global, out.row_offset = cs.x.shape[2], r0
    return out


_UNC_INTERPS = ("catmull", "linear", "linear")


# every (chain, dtype, plane, interp) the GPU tests stage: test_pairs_ingest_host.py asserts the mask condition on each
def reference_cases():
    out = []
    for k, chain in enumerate(CHAINS):                       # fused against the float64 reference
        out.append((chain, ("u16", "u8")[k % 2], PLANES[k % 3], ("linear", "catmull")[k % 2]))
    for dtype in ("u8", "u16"):                              # fused against two launches
        for plane in PLANES:
            out.append(("four", dtype, plane, "linear"))
    out.append(("data", "u16", (12, 20), "linear"))
    for k, smode in enumerate(pr.STD_MODES):                 # uncertainties
        out.append((("black", "clamp_channels", "four")[k], ("u16", "u8", "u16")[k], PLANES[(k + 1) % 3], _UNC_INTERPS[k]))
    out.append(("black", "u16", (11, 32), "linear"))         # row bands on tile boundaries
    out.append(("clamp_channels", "u8", (13, 17), "catmull"))  # a band cutting through tiles
    return sorted(set(out))


def uncertainty_cases():
    """(std mode, chain, dtype, plane, interp, layout): interleaved frames among them.  CATMULL meets the chain without a
    clamp only: a clamp bound inside the validity range parks a large share of the valid samples on ONE value, the float32
    Catmull-Rom derivative (a sum that cancels ~100x, ct_device.hpp) then carries the same rounding error in all of them, and
    the float32 eager oracle itself -- the reference's arithmetic -- leaves pr.TOL on such a stack (measured on the four-stage
    chain with explicit stds: 1.2x the tolerance of the weight sum).  pr.TOL is four times that oracle's deviation, so a case
    belongs here only if the oracle stays within a quarter of it: test_pairs_ingest_host.py asserts that for every case."""
    return [(smode, ("black", "clamp_channels", "four")[k], ("u16", "u8", "u16")[k], PLANES[(k + 1) % 3], _UNC_INTERPS[k],
             ("nhwc", "nchw", "nhwc_bgr")[k]) for k, smode in enumerate(pr.STD_MODES)]
