"""Time ct_strided_downscale alone against the torch expression a user would otherwise write,
``x.view(torch.int16)[..., ::s, ::s].contiguous()``, on the same device in the same process (profiles/downscale.md).

    python tools/downscale_bench.py [--batch 32] [--size 4096] [--launches 30] [--out FILE.json]

Per case: device-event time of every launch, the two candidates alternating, median after warm-up; the outputs are
compared for equality at the timed size.  The byte floor is what the gather cannot avoid: every selected source row
at full width (whole cache lines arrive while step * pixel_bytes is below the line size) plus the output, over the
8 TB/s HBM peak of the MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def _time(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    b, n = args.batch, args.size
    gen = torch.Generator(device=dev).manual_seed(1)
    flat = torch.randint(-32768, 32768, (b * 3 * n * n,), dtype=torch.int16, device=dev, generator=gen).view(torch.uint16)
    results = []
    for layout, shape in (("nchw", (b, 3, n, n)), ("nhwc", (b, n, n, 3))):
        x = flat.view(shape)
        for s in (2, 4):
            out = torch.empty(ops.downscaled_shape(shape, s, layout), dtype=torch.uint16, device=dev)
            if layout == "nchw":
                def torch_copy():
                    return x.view(torch.int16)[..., ::s, ::s].contiguous()
            else:
                def torch_copy():
                    return x.view(torch.int16)[:, ::s, ::s, :].contiguous()

            def kernel():
                return ops.strided_downscale(x, s, layout=layout, out=out)

            equal = bool(torch.equal(kernel().view(torch.int16), torch_copy()))
            t_k, t_t = [], []
            for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
                t_k += _time(kernel, 1, 0)
                t_t += _time(torch_copy, 1, 0)
            t_k, t_t = t_k[args.warmup:], t_t[args.warmup:]
            rows = -(-n // s)
            floor_bytes = b * 3 * rows * n * 2 + out.numel() * 2
            med_k, med_t = statistics.median(t_k), statistics.median(t_t)
            results.append({
                "case": f"uint16 {layout} {b}x3x{n}x{n} step {s}", "outputs_equal": equal,
                "launches": len(t_k), "kernel_ms_median": med_k * 1e3, "kernel_ms_min": min(t_k) * 1e3,
                "kernel_ms_max": max(t_k) * 1e3, "torch_ms_median": med_t * 1e3, "torch_ms_min": min(t_t) * 1e3,
                "torch_ms_max": max(t_t) * 1e3, "speedup_vs_torch": med_t / med_k, "floor_bytes": floor_bytes,
                "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "kernel_floor_TBps": floor_bytes / med_k / 1e12,
                "kernel_share_of_floor": floor_bytes / HBM_PEAK / med_k})
            print(json.dumps(results[-1]), flush=True)
            del out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
