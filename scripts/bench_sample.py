"""sample.lua:80-89 for one run -- 1024 images, D's score for each, the 64 best and the 64 worst laid out as 8 x 8 grids -- timed two ways
in one process, alternating:
  (a) host-driven, module level: nn_utils.createImages(1024) + sortImagesByPrediction(images, false, 64) +
      sortImagesByPrediction(images, true, 64) (every chunk through host tensors, D over all images twice, sort on the host);
  (b) sampler level: Sampler.sample(1024) + the two 64-image grids, each copied to the host.
BASELINE config-2 nets (create_G / create_D at 3x32x32), evaluate mode, chunk = --chunks (sample.lua's default 16, and 128).
usage: python scripts/bench_sample.py [--chunks 16,128] [--repeats 7] [--min-ms 300]      -> one JSON line per chunk size
       python scripts/bench_sample.py --kernels 1024,65536     # only launches fg_rank_scores / fg_image_grid at those n (for a
                                                               # rocprofv3 --kernel-trace --stats run of its own)
Every timing is a host clock between two device synchronisations over enough calls to fill --min-ms; every chunk shape is warmed up
first.  (profiles/r08_sample.md holds the figures.)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                     # noqa: E402
from face_generator_amd import models, nn_utils                  # noqa: E402
from face_generator_amd.runtime import get_context, Sampler      # noqa: E402
from face_generator_amd.state import S                           # noqa: E402

N, K = 1024, 64


def build(ctx, chunk):
    gen = torch.Generator().manual_seed(3)
    G, D = models.create_G((3, 32, 32), 100), models.create_D((3, 32, 32))
    nn_utils.initializeWeights(D, 0.05, 0.01, gen=gen)
    nn_utils.initializeWeights(G, 0.05, 0.01, gen=gen)
    S.reset()
    S.OPT.update(batchSize=chunk, noiseDim=100)
    S.MODEL_G = nn_utils.activateCuda(G, max_batch=chunk)
    S.MODEL_D = nn_utils.activateCuda(D, max_batch=chunk)
    nn_utils.switchToEvaluationMode()
    sm = Sampler(ctx, G._inner().device_net, D._inner().device_net, N, chunk)
    return sm


def host_driven():
    images = nn_utils.createImages(N)
    best, _ = nn_utils.sortImagesByPrediction(images, False, K)
    worst, _ = nn_utils.sortImagesByPrediction(images, True, K)
    return best, worst


def on_device(sm):
    sm.sample(N)
    return sm.grid("ORDER_DESC", K, 8).cpu(), sm.grid("ORDER_ASC", K, 8).cpu()


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def calls_for(fn, min_ms):
    one = timed(fn, 1)
    return max(1, int(min_ms / one + 0.999))


def summary(ms):
    med = statistics.median(ms)
    return dict(ms=round(med, 3), images_per_s=round(N / med * 1e3, 1), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                spread_pct=round(100.0 * (max(ms) - min(ms)) / med, 2))


def bench(ctx, chunk, repeats, min_ms):
    sm = build(ctx, chunk)
    a, b = host_driven, lambda: on_device(sm)
    for fn in (a, b, a, b):                                      # every chunk shape (full and tail) of both paths, twice
        fn()
    na, nb = calls_for(a, min_ms), calls_for(b, min_ms)
    ms_a, ms_b = [], []
    for _ in range(repeats):                                     # alternated: both paths see the same drift of the box
        ms_a.append(timed(a, na))
        ms_b.append(timed(b, nb))
    return dict(chunk=chunk, images=N, grid_images=K, repeats=repeats, calls_per_timing=dict(host_driven=na, sampler=nb),
                host_driven=summary(ms_a), sampler=summary(ms_b),
                speedup=round(statistics.median(ms_a) / statistics.median(ms_b), 3))


def kernels(ctx, sizes):
    for n in sizes:
        scores = ctx.uniform((n,), 0.0, 1.0, seed=5)
        order = torch.empty(n, dtype=torch.int32, device=ctx.device)
        imgs = ctx.uniform((n, 32, 32, 3), 0.0, 1.0, seed=6)
        nrow = 32 if n <= 1024 else 256
        grid = ctx.empty(3, -(-n // nrow) * 32, nrow * 32)
        for _ in range(5):
            for asc in (0, 1):
                ctx.check(ctx.lib.fg_rank_scores(ctx.h, scores.data_ptr(), n, asc, order.data_ptr(), None, 0))
            ctx.check(ctx.lib.fg_image_grid(ctx.h, imgs.data_ptr(), order.data_ptr(), n, 3, 32, 32, nrow, 0, 1, grid.data_ptr(), None))
        ctx.sync()
        print(json.dumps(dict(kernels_at_n=n, rank_launches=10, grid_launches=5, rank_grid=[-(-n // 256), 1],
                              minmax_grid=min(n, 256), fill_grid=-(-grid.numel() // 256))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="16,128")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--kernels", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sample.py: no HIP device -- timings are taken on the GPU only")
    ctx = get_context(0)
    if a.kernels:
        kernels(ctx, [int(v) for v in a.kernels.split(",")])
        return
    for chunk in (int(v) for v in a.chunks.split(",")):
        print(json.dumps(bench(ctx, chunk, a.repeats, a.min_ms)), flush=True)


if __name__ == "__main__":
    main()
