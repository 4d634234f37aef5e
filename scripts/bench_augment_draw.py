"""Times the draw of augmentation transforms on the device (fg_draw_transforms, runtime.DeviceAugmenter) beside the host draw it
replaces (runtime.Augmenter) -- the sibling of scripts/bench_augment.py and scripts/bench_train_loop.py, whose workloads and timing
helpers it uses.

    python scripts/bench_augment_draw.py [--only kernel|cfg2|c2f|all] [--rounds 5] [--min_ms 300] [--set 4096] [--repeats 50]

Kernel: fg_draw_transforms of n = 64 and n = 8192 transforms (the reference's ranges, 32 x 32) and the fg_warp_images launch it feeds
(a 65536 x 3x32x32 set, NCHW -> NHWC), device events around each repeat, alternating in one process, medians; the host draw of the
same n by Augmenter.draw plus its upload, wall clock, for scale.  Loops: adversarial.train at BASELINE configs[1] (32x32x3, batch 128)
and adversarial_c2f.train at configs[3] (64x64, batch 128), each on an un-augmented resident set, on a set augmented by the host
Augmenter and on one augmented by the DeviceAugmenter, alternating in one process, "time to learn 1 sample" as bench_train_loop.py
takes it.  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_train_loop as TL  # noqa: E402  (puts the package on the path too)


def bench_kernel(ctx, a):
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    n_set, c, hh, w = 65536, 3, 32, 32
    gen = torch.Generator(device=dev).manual_seed(1)
    images = torch.rand((n_set, c, hh, w), generator=gen, device=dev)
    P = lambda t: t.data_ptr()
    res = dict(n_set=n_set, image=[c, hh, w], repeats=a.repeats)
    for n in (64, 8192):
        idx = torch.randint(0, n_set, (n,), generator=gen, device=dev, dtype=torch.int32)
        out = torch.empty((n, hh, w, c), device=dev)
        aug, host = DeviceAugmenter((hh, w)), Augmenter((hh, w))
        both = aug.draw_device(ctx, n, (hh, w))
        paths = dict(draw=lambda: aug.draw_device(ctx, n, (hh, w)),
                     warp=lambda: ctx.check(lib.fg_warp_images(h, P(images), n_set, c, hh, w, 1, P(idx), P(both), P(both) + 24 * n, n, P(out), hh, w, 0, 0)))
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
        r = {}
        for k, t in times.items():
            r[k + "_us"] = round(statistics.median(t) * 1e3, 3)
            r[k + "_us_min"] = round(min(t) * 1e3, 3)
        # the host's side of the same hand-over: wall clock of the call (Python, ctypes, launch) and of the draw it replaces
        wall = dict(device_call=[], host_draw_and_upload=[])
        for _ in range(max(5, a.repeats // 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aug.draw_device(ctx, n, (hh, w))
            wall["device_call"].append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m, g = host.draw(n, (hh, w))
            torch.cat([torch.from_numpy(m).reshape(-1), torch.from_numpy(g)]).to(dev)
            torch.cuda.synchronize()
            wall["host_draw_and_upload"].append(time.perf_counter() - t0)
        for k, t in wall.items():
            r[k + "_wall_us"] = round(statistics.median(t) * 1e6, 1)
        res["n=%d" % n] = r
    return res


def three_way(ctx, train, sets, B, a):
    n_epoch = 4 * B
    for data in sets.values():
        TL.timed_epoch(ctx, train, data, n_epoch)
    while any(TL.timed_epoch(ctx, train, d, n_epoch) * n_epoch < a.min_ms for d in sets.values()):
        n_epoch *= 2
    t = {k: [] for k in sets}
    for _ in range(a.rounds):
        for k, d in sets.items():
            t[k].append(TL.timed_epoch(ctx, train, d, n_epoch))
    out = dict(batch=B, N_epoch=n_epoch, rounds=a.rounds)
    for k, v in t.items():
        med = statistics.median(v)
        out[k + "_ms_per_sample"] = round(med, 6)
        out[k + "_spread"] = round((max(v) - min(v)) / med, 4)
        out[k + "_epoch_ms"] = round(med * n_epoch, 2)
        out[k + "_all"] = [round(x, 6) for x in v]
    out["host_drawn_over_resident"] = round(out["host_drawn_ms_per_sample"] / out["resident_ms_per_sample"], 4)
    out["device_drawn_over_resident"] = round(out["device_drawn_ms_per_sample"] / out["resident_ms_per_sample"], 4)
    out["device_drawn_over_host_drawn"] = round(out["device_drawn_ms_per_sample"] / out["host_drawn_ms_per_sample"], 4)
    return out


def bench_cfg2(ctx, a):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter, DeviceDataset
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
    sets = dict(resident=DeviceDataset(ctx, images), host_drawn=DeviceDataset(ctx, images, augment=Augmenter(dims[1:])),
                device_drawn=DeviceDataset(ctx, images, augment=DeviceAugmenter(dims[1:])))
    return three_way(ctx, adversarial.train, sets, B, a)


def bench_c2f(ctx, a):
    from face_generator_amd import models_c2f, adversarial_c2f, dataset_c2f
    from face_generator_amd.runtime import Augmenter, DeviceAugmenter
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
    sets = dict(resident=dataset_c2f.toResultResident(fine, Sz // 2, Sz, ctx=ctx),
                host_drawn=dataset_c2f.toResultAugmented(fine, Sz // 2, Sz, Augmenter((Sz, Sz)), ctx=ctx),
                device_drawn=dataset_c2f.toResultAugmented(fine, Sz // 2, Sz, DeviceAugmenter((Sz, Sz)), ctx=ctx))
    return three_way(ctx, adversarial_c2f.train, sets, B, a)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("kernel", "cfg2", "c2f", "all"), default="all")
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
    if a.only in ("kernel", "all"):
        out["kernel"] = bench_kernel(ctx, a)
    if a.only in ("cfg2", "all"):
        out["cfg2_adversarial_train"] = bench_cfg2(ctx, a)
    if a.only in ("c2f", "all"):
        out["c2f_adversarial_c2f_train"] = bench_c2f(ctx, a)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
