"""Times the per-batch augmentation of a set resident in HBM (fg_warp_images, runtime.Augmenter) beside the plain gather
(fg_gather_images) -- the sibling of scripts/bench_train_loop.py, whose workloads and timing helpers it uses.

    python scripts/bench_augment.py [--only kernel|loops|both] [--rounds 5] [--min_ms 300] [--set 4096] [--repeats 50]

Kernel: a 65536 x 3x32x32 set, 8192 random indices, NCHW -> NHWC, matrices and gains drawn by Augmenter((32, 32)); device events
around each repeat, warp and gather alternating in one process, medians.  Both move the same bytes: n * c * h * w * 4 read and as
many written (the warp reads 28 more bytes per image: its index, matrix and gain).  Per batch: n = 64 images, 100 launches between two
events, per launch.  Loops: adversarial.train at BASELINE configs[1] (32x32x3, batch 128) on a DeviceDataset with and without an
Augmenter, alternating, "time to learn 1 sample" as bench_train_loop.py takes it.  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_train_loop as TL  # noqa: E402  (puts the package on the path too)


def bench_kernel(ctx, a):
    from face_generator_amd.runtime import Augmenter
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    n_set, c, hh, w, n = 65536, 3, 32, 32, 8192
    gen = torch.Generator(device=dev).manual_seed(1)
    images = torch.rand((n_set, c, hh, w), generator=gen, device=dev)
    idx = torch.randint(0, n_set, (n,), generator=gen, device=dev, dtype=torch.int32)
    mats_h, gains_h = Augmenter((hh, w)).draw(n, (hh, w))
    mats, gains = torch.from_numpy(mats_h).to(dev), torch.from_numpy(gains_h).to(dev)
    out, out2 = torch.empty((n, hh, w, c), device=dev), torch.empty((n, hh, w, c), device=dev)
    nbytes = out.numel() * 4
    P = lambda t: t.data_ptr()

    def warp(count=n, m=mats, g=gains, fill=0, o=out, layout=0):
        ctx.check(lib.fg_warp_images(h, P(images), n_set, c, hh, w, 1, P(idx), None if m is None else P(m), None if g is None else P(g), count,
                                     P(o), hh, w, layout, fill))

    def gather(count=n):
        ctx.check(lib.fg_gather_images(h, P(images), n_set, c, hh, w, 1, P(idx), count, P(out2), 0))
    paths = dict(warp=warp, gather=gather, warp_edge=lambda: warp(fill=1), warp_identity=lambda: warp(m=None, g=None),
                 warp_rows=lambda: warp(layout=1))
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
    res["warp_over_gather"] = round(res["warp_ms"] / res["gather_ms"], 3)
    # per batch: 64 images, 100 launches between two events
    per = {}
    for k, f in (("warp", lambda: warp(64)), ("gather", lambda: gather(64))):
        for _ in range(10):
            f()
        torch.cuda.synchronize()
        t = []
        for _ in range(max(5, a.repeats // 5)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                f()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / 100)
        per[k + "_us_per_launch"] = round(statistics.median(t) * 1e3, 3)
    res["batch_of_64"] = per
    # the results at the timed size: the identity is the gather, bit for bit
    warp(m=None, g=None)
    gather()
    torch.cuda.synchronize()
    res["identity_equals_gather"] = bool(torch.equal(out.view(torch.int32), out2.view(torch.int32)))
    return res


def bench_loops(ctx, a):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import Augmenter, DeviceDataset
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
    sets = dict(resident=DeviceDataset(ctx, images), augmented=DeviceDataset(ctx, images, augment=Augmenter(dims[1:])))
    n_epoch = 4 * B
    for data in sets.values():
        TL.timed_epoch(ctx, adversarial.train, data, n_epoch)
    while any(TL.timed_epoch(ctx, adversarial.train, d, n_epoch) * n_epoch < a.min_ms for d in sets.values()):
        n_epoch *= 2
    t = {k: [] for k in sets}
    for _ in range(a.rounds):
        for k, d in sets.items():
            t[k].append(TL.timed_epoch(ctx, adversarial.train, d, n_epoch))
    out = dict(batch=B, N_epoch=n_epoch, rounds=a.rounds)
    for k, v in t.items():
        med = statistics.median(v)
        out[k + "_ms_per_sample"] = round(med, 6)
        out[k + "_spread"] = round((max(v) - min(v)) / med, 4)
        out[k + "_all"] = [round(x, 6) for x in v]
    out["augmented_over_resident"] = round(out["augmented_ms_per_sample"] / out["resident_ms_per_sample"], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("kernel", "loops", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=300.0)
    ap.add_argument("--set", type=int, default=4096, help="images of the synthetic 32-px set")
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args(argv)
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    random.seed(1)
    out = dict(device=torch.cuda.get_device_name(0))
    if a.only in ("kernel", "both"):
        out["kernel"] = bench_kernel(ctx, a)
    if a.only in ("loops", "both"):
        out["cfg2_adversarial_train"] = bench_loops(ctx, a)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
