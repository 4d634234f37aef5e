"""Times the nearest-neighbour search of `sample --neighbours` on the device: q = 16 queries against a resident set of 65536 x 3072
floats (the 32-px RGB images of sample.lua), one fg_nearest_update call, beside the only way the library could do it before that
entry existed: 16 calls of fg_parzen_min_dist over the same rows with a zero `cond`, each reading the whole set.

    python scripts/bench_neighbours.py [--only new|baseline|both] [--rows 65536] [--elems 3072] [--q 16] [--repeats 30] [--warmup 5]

Device events around each repeat, medians over the repeats; the two paths alternate inside one process.  `--only baseline` needs
nothing but fg_parzen_min_dist, so it also runs against an older build of the library (put that build's package first on
PYTHONPATH).  Prints one JSON line.  Bytes and operations are counted from the shapes:
  row stream   rows * elems * 4 bytes, read once by the new path and q times by the baseline;
  fp64 work    rows * elems * q element pairs, each one fp32 subtract, one fp32 -> fp64 convert and one fp64 FMA; `fp64_share` is
               the time the convert and the FMA need at the vector fp64 peak (2 instructions of fp64 rate per pair, --fp64_tflops
               counts an FMA as 2 FLOP) over the measured time -- a computed bound, not a counter reading."""
import argparse
import json
import os
import statistics
import sys

import torch

try:
    import face_generator_amd  # noqa: F401  (a build put first on PYTHONPATH wins)
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("new", "baseline", "both"), default="both")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--elems", type=int, default=3072)
    ap.add_argument("--q", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fp64_tflops", type=float, default=78.6, help="vector fp64 peak of the device (MI355X data sheet: 78.6)")
    a = ap.parse_args(argv)
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    n, elems, q = a.rows, a.elems, a.q
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = torch.rand((n, elems), generator=gen, device=dev)
    queries = torch.rand((q, elems), generator=gen, device=dev)
    P = lambda t: t.data_ptr()
    paths = {}
    if a.only in ("new", "both"):
        if not hasattr(lib, "fg_nearest_update"):
            raise SystemExit("this build of the library has no fg_nearest_update: use --only baseline")
        nb = lib.fg_nearest_workspace_bytes(q, n)
        scratch = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        d2 = torch.empty(q, dtype=torch.float64, device=dev)
        idx = torch.empty(q, dtype=torch.int32, device=dev)
        dist = torch.empty(q, device=dev)
        paths["new"] = lambda: ctx.check(lib.fg_nearest_update(h, P(queries), q, P(rows), n, elems, 0, 1, P(d2), P(idx), P(dist), P(scratch), nb))
    if a.only in ("baseline", "both"):
        cond = torch.zeros(elems, device=dev)
        bdist = torch.empty((q, n), device=dev)
        bmin = torch.empty(q, device=dev)

        def baseline():
            for j in range(q):
                ctx.check(lib.fg_parzen_min_dist(h, P(rows), P(cond), P(queries[j]), n, elems, P(bdist[j]), P(bmin[j:])))
        paths["baseline"] = baseline
    for _ in range(a.warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, f in paths.items():                       # alternating: both paths see the same clocks and neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    out = dict(rows=n, elems=elems, q=q, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    stream = n * elems * 4
    for k, t in times.items():
        ms = statistics.median(t)
        out[k + "_ms"] = round(ms, 4)
        out[k + "_ms_min"] = round(min(t), 4)
        out[k + "_row_bytes_read"] = stream * (1 if k == "new" else q)
        out[k + "_row_stream_TBps"] = round(out[k + "_row_bytes_read"] / (ms * 1e-3) / 1e12, 3)
    if "new" in times:
        fp64_ms = 2.0 * n * elems * q / (a.fp64_tflops * 1e12 / 2.0) * 1e3
        out["new_fp64_ms_at_peak"] = round(fp64_ms, 4)
        out["new_fp64_share"] = round(fp64_ms / out["new_ms"], 3)
    if len(times) == 2:
        out["speedup"] = round(out["baseline_ms"] / out["new_ms"], 2)
        # same answer: the baseline's arg-min on the host against the new entry's
        got, want = idx.cpu(), bdist.argmin(dim=1).cpu().to(torch.int32)
        out["same_indices"] = bool(torch.equal(got, want))
        out["max_rel_dist_diff"] = float(((dist - bdist.min(dim=1).values).abs() / dist).max())
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
