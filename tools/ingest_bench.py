"""Time ct_ingest_transform alone against the torch chain the staging ran before it existed -- the transform classes'
``__call__`` on the device tensor, then ``.to(float32).contiguous()`` -- on the same device in the same process
(profiles/ingest.md).

    python tools/ingest_bench.py [--launches 30] [--warmup 5] [--out FILE.json] [--data-dependent]

The list is ``[CastTo(float32), Normalize(4095, 64), ClampAlongDims(1, 3 pairs)]``, behind ``CvToTorch`` for the raw
(B,H,W,3) BGR frames.  Per case: device-event time of every run, the two candidates alternating, median after warm-up.
The byte floor is ``sizeof(T) + 4`` bytes per sample, every byte once, over the 8 TB/s HBM peak of the MI355X.  The
outputs are also compared: ``differing`` counts the elements of the torch chain's result whose bits are not the fused
pass's (which the tests pin to the CPU reference), i.e. the rounding gap of the torch route on the device.

``--data-dependent`` (profiles/ingest_data.md): the list is ``[CastTo(float32), Normalize()]`` -- the batch's own
extrema -- and the candidates are ``ops.ingest_transform_data(check=False)`` (ct_ingest_extrema, its fold and
ct_ingest_transform_data) against the same torch chain; the extrema pass is also timed alone, against its own floor of
``sizeof(T)`` bytes per sample.  Both candidates' zero-range check (one readback each) is left out of the timing.  A
small stack is additionally run through the torch route on the device and through the classes on the CPU, and the
elements whose bits differ are counted (``torch_route_vs_cpu_differing``).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402
from clair_torch_amd.common.transforms import (CastTo, ClampAlongDims, CvToTorch, Normalize, fusable_ingest,  # noqa: E402
                                               fusable_ingest_data)

HBM_PEAK = 8.0e12  # bytes / s
PAIRS = [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)]
CASES = [((32, 3, 4096, 4096), torch.uint16, 4500), ((64, 3, 1080, 1920), torch.uint8, 255)]


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _draw(shape, dtype, top, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.uint16:  # torch draws no uint16: the codes fit the positive half of int16
        return torch.randint(0, top + 1, shape, dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    return torch.randint(0, top + 1, shape, dtype=dtype, device=dev, generator=gen)


def data_dependent(args, dev):
    """[CastTo(float32), Normalize()]: extrema + ingest against the torch chain; the extrema pass alone."""
    results = []
    for (b, c, h, w), dtype, top in CASES:
        for layout in ("nchw", "nhwc_bgr"):
            shape = (b, c, h, w) if layout == "nchw" else (b, h, w, c)
            x = _draw(shape, dtype, top, dev)
            ts = ([CvToTorch()] if layout != "nchw" else []) + [CastTo("float32"), Normalize()]
            plan = fusable_ingest_data(x, ts)
            assert plan is not None and plan.layout == layout and plan.prefix == ()
            out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)

            def fused():
                return ops.ingest_transform_data(x, plan.stages, layout, check=False, out=out)

            def extrema():
                return ops.ingest_extrema(x, (), layout)

            def torch_chain():
                y = x
                for t in ts[:-1]:
                    y = t(y)
                lo, hi = y.min(), y.max()   # Normalize.__call__ without its ``den == 0`` readback
                return ((y - lo) / (hi - lo) * 1.0 + 0.0).to(torch.float32).contiguous()

            ref = torch_chain()
            differing = int((fused()[0].view(torch.int32) != ref.view(torch.int32)).sum())
            del ref
            t_f, t_e, t_t = [], [], []
            for _ in range(args.launches):  # alternate the candidates: all see the same neighbours and clocks
                t_f.append(_time(fused))
                t_e.append(_time(extrema))
                t_t.append(_time(torch_chain))
            t_f, t_e, t_t = t_f[args.warmup:], t_e[args.warmup:], t_t[args.warmup:]
            read = x.numel() * x.element_size()
            floor_bytes = 2 * read + 4 * x.numel()   # the stack is read twice (extrema, ingest) and written once as float32
            med_f, med_e, med_t = statistics.median(t_f), statistics.median(t_e), statistics.median(t_t)
            row = {"case": f"{b}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {layout}", "launches": len(t_f),
                   "fused_ms_median": med_f * 1e3, "fused_ms_min": min(t_f) * 1e3, "fused_ms_max": max(t_f) * 1e3,
                   "extrema_ms_median": med_e * 1e3, "extrema_ms_min": min(t_e) * 1e3, "extrema_ms_max": max(t_e) * 1e3,
                   "torch_ms_median": med_t * 1e3, "torch_ms_min": min(t_t) * 1e3, "torch_ms_max": max(t_t) * 1e3,
                   "speedup_vs_torch": med_t / med_f, "extrema_bytes": read, "extrema_floor_ms_at_8TBps": read / HBM_PEAK * 1e3,
                   "extrema_TBps": read / med_e / 1e12, "fused_floor_bytes": floor_bytes,
                   "fused_floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "fused_TBps": floor_bytes / med_f / 1e12,
                   "elements": x.numel(), "differing": differing}
            results.append(row)
            print(json.dumps(row), flush=True)
            del x, out
            torch.cuda.empty_cache()
    # the torch route on the device against the classes on the CPU: is it bit-identical for this list?
    for dtype, top in ((torch.uint16, 4500), (torch.uint8, 255)):
        x = _draw((4, 3, 256, 512), dtype, top, dev)
        ts = [CastTo("float32"), Normalize()]
        on_dev, on_cpu = x, x.cpu()
        for t in ts:
            on_dev, on_cpu = t(on_dev), t(on_cpu)
        fused = ops.ingest_transform_data(x, [("affine_data", 1.0, 0.0)])
        row = {"case": f"4x3x256x512 {str(dtype).split('.')[-1]} nchw, torch route on the device vs the classes on the CPU",
               "elements": x.numel(),
               "torch_route_vs_cpu_differing": int((on_dev.cpu().view(torch.int32) != on_cpu.view(torch.int32)).sum()),
               "fused_vs_cpu_differing": int((fused.cpu().view(torch.int32) != on_cpu.view(torch.int32)).sum())}
        results.append(row)
        print(json.dumps(row), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--data-dependent", action="store_true", help="[CastTo, Normalize()]: extrema + ingest (profiles/ingest_data.md)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    dev = torch.device("cuda:0")
    results = data_dependent(args, dev) if args.data_dependent else []
    for (b, c, h, w), dtype, top in ([] if args.data_dependent else CASES):
        for layout in ("nchw", "nhwc_bgr"):
            shape = (b, c, h, w) if layout == "nchw" else (b, h, w, c)
            x = _draw(shape, dtype, top, dev)
            ts = [CastTo("float32"), Normalize(4095 if dtype == torch.uint16 else 255, 64 if dtype == torch.uint16 else 16),
                  ClampAlongDims(1, PAIRS)]
            ts = ([CvToTorch()] if layout != "nchw" else []) + ts
            plan = fusable_ingest(x, ts)
            assert plan is not None and plan.layout == layout
            out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)

            def kernel():
                return ops.ingest_transform(x, plan.stages, layout=layout, out=out)

            def torch_chain():
                y = x
                for t in ts:
                    y = t(y)
                return y.to(torch.float32).contiguous()

            ref = torch_chain()
            differing = int((kernel().view(torch.int32) != ref.view(torch.int32)).sum())
            del ref
            t_k, t_t = [], []
            for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
                t_k.append(_time(kernel))
                t_t.append(_time(torch_chain))
            t_k, t_t = t_k[args.warmup:], t_t[args.warmup:]
            floor_bytes = x.numel() * (x.element_size() + 4)
            med_k, med_t = statistics.median(t_k), statistics.median(t_t)
            row = {"case": f"{b}x{c}x{h}x{w} {str(dtype).split('.')[-1]} {layout}", "launches": len(t_k),
                   "kernel_ms_median": med_k * 1e3, "kernel_ms_min": min(t_k) * 1e3, "kernel_ms_max": max(t_k) * 1e3,
                   "torch_ms_median": med_t * 1e3, "torch_ms_min": min(t_t) * 1e3, "torch_ms_max": max(t_t) * 1e3,
                   "speedup_vs_torch": med_t / med_k, "floor_bytes": floor_bytes,
                   "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "kernel_floor_TBps": floor_bytes / med_k / 1e12,
                   "kernel_share_of_floor": floor_bytes / HBM_PEAK / med_k, "elements": x.numel(),
                   "differing": differing}
            results.append(row)
            print(json.dumps(row), flush=True)
            del x, out
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
