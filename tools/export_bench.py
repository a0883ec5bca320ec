"""Time ct_export_cv alone against the torch expression a user would otherwise write before the device-to-host copy,
``x.permute(1, 2, 0).flip(-1).to(dtype).contiguous()`` (``permute(0, 2, 3, 1)`` for a stack), on the same device in the
same process (profiles/export.md).

    python tools/export_bench.py [--launches 30] [--warmup 5] [--host] [--out FILE.json]

Per case: device-event time of every launch, the two candidates alternating, median after warm-up; the outputs are
compared for equality at the timed size.  The byte floor is source plus destination, every byte once, over the 8 TB/s
HBM peak of the MI355X.  ``--host`` also times, once per case, what the reference's save_image does on the host with the
``.cpu()`` copy of the planar result (astype, transpose, fancy-index reversal; data_io.py:228-234).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clair_torch_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
_NAME = {torch.float32: "f32", torch.float64: "f64"}
CASES = [((3, 4096, 4096), torch.float64, torch.float64),   # C2 mean
         ((3, 4096, 4096), torch.float64, torch.float32),
         ((3, 4096, 4096), torch.float32, torch.float32),   # C2 std
         ((16, 3, 1080, 1920), torch.float32, torch.float32)]  # one C4 group


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _host_expression(array, dtype):
    array = array.astype(dtype=dtype)
    array = np.transpose(array, (1, 2, 0))
    return array[:, :, [2, 1, 0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    assert args.launches - args.warmup >= 25, "the median is taken over at least 25 launches"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for shape, src, dst in CASES:
        x = torch.randn(shape, dtype=src, device=dev, generator=gen)
        out = torch.empty(ops.export_shape(shape), dtype=dst, device=dev)
        perm = (1, 2, 0) if len(shape) == 3 else (0, 2, 3, 1)

        def torch_copy():
            return x.permute(*perm).flip(-1).to(dst).contiguous()

        def kernel():
            return ops.export_cv(x, dst, out=out)

        equal = bool(torch.equal(kernel(), torch_copy()))
        t_k, t_t = [], []
        for _ in range(args.launches):  # alternate the candidates: both see the same neighbours and clocks
            t_k.append(_time(kernel))
            t_t.append(_time(torch_copy))
        t_k, t_t = t_k[args.warmup:], t_t[args.warmup:]
        floor_bytes = x.numel() * x.element_size() + out.numel() * out.element_size()
        med_k, med_t = statistics.median(t_k), statistics.median(t_t)
        row = {
            "case": f"{'x'.join(map(str, shape))} {_NAME[src]}->{_NAME[dst]}", "outputs_equal": equal,
            "launches": len(t_k), "kernel_ms_median": med_k * 1e3, "kernel_ms_min": min(t_k) * 1e3,
            "kernel_ms_max": max(t_k) * 1e3, "torch_ms_median": med_t * 1e3, "torch_ms_min": min(t_t) * 1e3,
            "torch_ms_max": max(t_t) * 1e3, "speedup_vs_torch": med_t / med_k, "floor_bytes": floor_bytes,
            "floor_ms_at_8TBps": floor_bytes / HBM_PEAK * 1e3, "kernel_floor_TBps": floor_bytes / med_k / 1e12,
            "kernel_share_of_floor": floor_bytes / HBM_PEAK / med_k}
        if args.host:
            images = x.cpu().numpy()
            images = images[None] if images.ndim == 3 else images
            t0 = time.perf_counter()
            host = [_host_expression(a, np.dtype(_NAME[dst].replace("f", "float"))) for a in images]
            row["host_expression_ms_once"] = (time.perf_counter() - t0) * 1e3
            row["host_equal"] = bool(np.array_equal(np.stack(host).reshape(out.shape), out.cpu().numpy()))
            del host, images
        results.append(row)
        print(json.dumps(row), flush=True)
        del x, out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
