"""Times the epoch loops themselves -- adversarial.train at BASELINE configs[1] (32x32x3, batch 128) and adversarial_c2f.train at
configs[3] (64x64, batch 128) -- fed from a host dataset (dataset[i] per image, stack, upload, layout kernel) and from a set
resident in HBM (runtime.DeviceDataset / dataset_c2f.toResultResident: one fg_gather_images per batch), and the gather kernel alone
beside a device-to-device copy of the same bytes.  bench.py times neither: its inputs are resident before the clock starts.

    python scripts/bench_train_loop.py [--only loops|gather|both] [--rounds 5] [--min_ms 300] [--set 4096] [--repeats 50]

Loops: synthetic images, fresh nets per workload, N_epoch grown until one epoch runs for at least --min_ms; then --rounds rounds,
each one host-fed epoch and one resident epoch (alternating, one process: both see the same clocks and neighbours).  The number is
the loop's own "time to learn 1 sample" (wall clock around train(), device drained, over N_epoch); medians, and the spread as
(max - min) / median.  Gather: a 65536 x 3x32x32 set, 8192 random indices, NCHW -> NHWC, device events around each repeat, median;
fg_d2d of the same number of output bytes in the same process is the yardstick.  Bytes: the gather reads and writes
n * c * h * w * 4 each (plus 4 * n of indices), and so does the copy.  Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

try:
    import face_generator_amd  # noqa: F401  (a build put first on PYTHONPATH wins)
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class ListDataset:
    """dataset[i] -> host CHW array, dataset.size(): the host-fed protocol of adversarial.train"""

    def __init__(self, items):
        self.items = items

    def size(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def timed_epoch(ctx, train, data, n_epoch):
    """-> ms per sample of one epoch (the loop's own figure, with the device drained at both ends)"""
    from face_generator_amd.state import S
    S.OPT["N_epoch"] = n_epoch
    ctx.sync()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        train(data)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / n_epoch


def loop_stats(ctx, train, host, resident, B, rounds, min_ms):
    n_epoch = 4 * B
    for data in (host, resident):                            # warm-up: plans, workspaces, allocator
        timed_epoch(ctx, train, data, n_epoch)
    while timed_epoch(ctx, train, host, n_epoch) * n_epoch < min_ms or timed_epoch(ctx, train, resident, n_epoch) * n_epoch < min_ms:
        n_epoch *= 2
    t = dict(host=[], resident=[])
    for _ in range(rounds):
        t["host"].append(timed_epoch(ctx, train, host, n_epoch))
        t["resident"].append(timed_epoch(ctx, train, resident, n_epoch))
    out = dict(batch=B, N_epoch=n_epoch, rounds=rounds)
    for k, v in t.items():
        med = statistics.median(v)
        out[k + "_ms_per_sample"] = round(med, 6)
        out[k + "_spread"] = round((max(v) - min(v)) / med, 4)
        out[k + "_epoch_ms"] = round(med * n_epoch, 2)
        out[k + "_all"] = [round(x, 6) for x in v]
    out["resident_over_host"] = round(out["resident_ms_per_sample"] / out["host_ms_per_sample"], 4)
    return out


def bench_cfg2(ctx, a):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import DeviceDataset
    from face_generator_amd.state import S
    B, dims = 128, (3, 32, 32)
    S.reset()
    adversarial.accs.clear()
    S.OPT.update(batchSize=B, noiseDim=100, saveFreq=10 ** 9, seed=1, scale=32)
    S.IMG_DIMENSIONS = dims
    torch.manual_seed(1)
    S.MODEL_G = nn_utils.activateCuda(models.create_G(dims, 100))
    S.MODEL_D = nn_utils.activateCuda(models.create_D(dims))
    S.set_dist(None)
    images = np.random.default_rng(1).uniform(0, 1, (a.set,) + dims).astype(np.float32)
    return loop_stats(ctx, adversarial.train, ListDataset(list(images)), DeviceDataset(ctx, images), B, a.rounds, a.min_ms)


def bench_c2f(ctx, a):
    from face_generator_amd import models_c2f, adversarial_c2f, dataset_c2f
    from face_generator_amd.state import S
    B, Sz = 128, 64
    S.reset()
    S.OPT.update(batchSize=B, saveFreq=10 ** 9, seed=1, coarseSize=Sz // 2, fineSize=Sz)
    S.IMG_DIMENSIONS = (3, Sz, Sz)
    torch.manual_seed(1)
    S.MODEL_G = models_c2f.create_G((3, Sz, Sz), cuda=True, max_batch=B)
    S.MODEL_D = models_c2f.create_D((3, Sz, Sz), cuda=True, max_batch=B)
    S.set_dist(None)
    S._trainer = adversarial_c2f.TrainerC2F(ctx, S.MODEL_G, S.MODEL_D, S.OPT)
    fine = torch.tensor(np.random.default_rng(2).uniform(0, 1, (a.set // 2, 3, Sz, Sz)).astype(np.float32))
    host = dataset_c2f.toResult(fine, Sz // 2, Sz, ctx=ctx)
    resident = dataset_c2f.toResultResident(fine, Sz // 2, Sz, ctx=ctx)
    return loop_stats(ctx, adversarial_c2f.train, host, resident, B, a.rounds, a.min_ms)


def bench_gather(ctx, a):
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    n_set, c, hh, w, n = 65536, 3, 32, 32, 8192
    gen = torch.Generator(device=dev).manual_seed(1)
    images = torch.rand((n_set, c, hh, w), generator=gen, device=dev)
    idx = torch.randint(0, n_set, (n,), generator=gen, device=dev, dtype=torch.int32)
    out = torch.empty((n, hh, w, c), device=dev)
    src = torch.rand((n, hh, w, c), generator=gen, device=dev)
    nbytes = out.numel() * 4
    P = lambda t: t.data_ptr()
    paths = dict(gather=lambda: ctx.check(lib.fg_gather_images(h, P(images), n_set, c, hh, w, 1, P(idx), n, P(out), 0)),
                 gather_rows=lambda: ctx.check(lib.fg_gather_images(h, P(images), n_set, c, hh, w, 1, P(idx), n, P(out), 1)),
                 d2d=lambda: ctx.check(lib.fg_d2d(h, P(out), P(src), nbytes)))
    for _ in range(5):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = dict(n_set=n_set, n=n, image=[c, hh, w], output_bytes=nbytes, repeats=a.repeats)
    for k, t in times.items():
        ms = statistics.median(t)
        res[k + "_ms"] = round(ms, 5)
        res[k + "_ms_min"] = round(min(t), 5)
        res[k + "_TBps_read_plus_write"] = round(2 * nbytes / (ms * 1e-3) / 1e12, 3)
    res["gather_over_d2d"] = round(res["gather_ms"] / res["d2d_ms"], 3)
    want = images[idx.long()].permute(0, 2, 3, 1).contiguous()
    paths["gather"]()
    res["gather_equals_indexing"] = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("loops", "gather", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=300.0)
    ap.add_argument("--set", type=int, default=4096, help="images of the synthetic 32-px set (the 64-px set holds half as many)")
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args(argv)
    if a.rounds < 5:
        raise SystemExit("--rounds: at least five alternations")
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    random.seed(1)
    out = dict(device=torch.cuda.get_device_name(0))
    if a.only in ("gather", "both"):
        out["gather"] = bench_gather(ctx, a)
    if a.only in ("loops", "both"):
        out["cfg2_adversarial_train"] = bench_cfg2(ctx, a)
        out["c2f_adversarial_c2f_train"] = bench_c2f(ctx, a)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
