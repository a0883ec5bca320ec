"""Host time per call of the fronts of clair_torch_amd.ops beside the HDR merge, this tree's ops.py against another version of the
file (the parent commit's, written out with ``git show <commit>:clair_torch_amd/ops.py``), on the CPU and without a GPU.

The method of profiles/merge_fronts_refactor.md: the library is replaced by an object whose every entry point returns 0,
``_require_device``, ``_stream`` and ``torch.cuda.device`` are patched as in tests/test_fronts_host.py, whose cases and inputs
(stacks of 2 x 3 x 4 x 6) are the workload.  Both versions are loaded into one process; per case CALLS calls per repeat, the two
versions alternating, one warm-up repeat dropped and REPEATS kept; microseconds per call.  One run is one session: run it several
times.  Prints one markdown table row per case: the other version's span and median, this tree's median, and the excess of that
median over the other version's slowest repeat where there is one.

    python tools/fronts_host_bench.py OTHER_OPS.py [case prefix ...]"""
import contextlib
import importlib.util
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_fronts_host as cases  # noqa: E402
from clair_torch_amd import ops as new_ops  # noqa: E402

CALLS, REPEATS = 2000, 5


class Library:
    """Every ``ct_*`` entry point returns 0, every ``ct_*_workspace`` the contract's workspace size."""

    def __getattr__(self, entry):
        if not entry.startswith("ct_"):
            raise AttributeError(entry)
        fn = (lambda *a: cases.WORKSPACE_BYTES) if entry.endswith("_workspace") else (lambda *a: 0)
        setattr(self, entry, fn)
        return fn


def _load(path):
    spec = importlib.util.spec_from_file_location("clair_torch_amd._ops_other", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _time(module, case, t):
    call = cases._CASES[case]      # (the cases take the module whose fronts they call)
    start = time.perf_counter()
    for _ in range(CALLS):
        call(module, t)
    return (time.perf_counter() - start) / CALLS * 1e6


def main():
    other = _load(sys.argv[1])
    prefixes = tuple(sys.argv[2:])
    lib = Library()
    new_ops.nv.load = lambda: lib
    torch.cuda.device = lambda device: contextlib.nullcontext()
    for module in (other, new_ops):
        module._require_device = lambda t, name: None
        module._stream = lambda device: None
    print("| case | other: min .. max (median) | this tree: median (min .. max) | above the other's slowest |")
    print("|---|---|---|---|")
    for case, record in cases._RECORDED.items():
        if not record["calls"] or (prefixes and not case.startswith(prefixes)):
            continue
        t, _ = cases._inputs()
        times = {other: [], new_ops: []}
        for repeat in range(REPEATS + 1):
            for module in (other, new_ops):
                us = _time(module, case, t)
                if repeat:
                    times[module].append(us)
        a, b = times[other], times[new_ops]
        excess = statistics.median(b) - max(a)
        print(f"| {case} | {min(a):.2f} .. {max(a):.2f} ({statistics.median(a):.2f}) | {statistics.median(b):.2f} "
              f"({min(b):.2f} .. {max(b):.2f}) | {f'+{excess:.2f} us' if excess > 0 else ''} |")


if __name__ == "__main__":
    main()
