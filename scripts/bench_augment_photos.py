"""Times the augmentation from photo-sized sources (fg_warp_faces, runtime.PhotoDataset, dataset_c2f.PhotoResult) beside the
un-augmented resident sets and the face-sized augmented sets (DeviceDataset / AugmentedResult + DeviceAugmenter) -- the sibling of
scripts/bench_augment_draw.py and scripts/bench_train_loop.py, whose workloads and timing helpers it uses.

    python scripts/bench_augment_photos.py [--only kernel|stages|cfg2|c2f|all] [--rounds 5] [--min_ms 300] [--set 1024] [--repeats 50]

Photos are synthetic, 250 x 250 x 3 (LFW's size), the face window 84 x 84.  Kernel: fg_warp_faces at the pull sizes of the training
loops at batch 128 -- 84 -> 32 without fields (n = 64), 84 -> 64 with cs = 32 for ("diff", "coarse") (n = 64) and for ("coarse",)
(n = 64 and n = 128) -- beside fg_warp_images (40 -> 32) and fg_warp_c2f (64 -> 64) at the same n and fields, device events around
each repeat, alternating in one process, fresh random indices every repeat (a pull of the loops meets photos that no cache holds),
min / median / max.  Stages: the same entry with stages left out by the choice of sizes
(bench_stages).  Loops: adversarial.train at BASELINE configs[1] (32x32x3, batch 128)
and adversarial_c2f.train at configs[3] (64x64, batch 128), each on the un-augmented resident set, on the face-sized set augmented by
a DeviceAugmenter and on a PhotoDataset / PhotoResult with a DeviceAugmenter, alternating in one process, "time to learn 1 sample" as
bench_train_loop.py takes it, min / median / max per leg.  Prints one JSON line."""
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

PHOTO, WINDOW = (3, 250, 250), (84, 84)


def photos_on_device(ctx, n):
    gen = torch.Generator(device=ctx.device).manual_seed(3)
    return torch.rand((n,) + PHOTO, generator=gen, device=ctx.device)


def min_med_max(values, scale=1.0, digits=3):
    return [round(min(values) * scale, digits), round(statistics.median(values) * scale, digits), round(max(values) * scale, digits)]


def bench_kernel(ctx, a):
    from face_generator_amd.runtime import DeviceAugmenter
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    gen = torch.Generator(device=dev).manual_seed(1)
    photos = photos_on_device(ctx, a.set)
    c = PHOTO[0]
    set40, set64 = torch.rand((a.set, c, 40, 40), generator=gen, device=dev), torch.rand((a.set, c, 64, 64), generator=gen, device=dev)
    P = lambda t: None if t is None else t.data_ptr()
    res = dict(n_photos=a.set, photo=list(PHOTO), window=list(WINDOW), repeats=a.repeats, order="min, median, max (us)")
    for name, n, s, cs, fields in (("84->32 fine n=64", 64, 32, 0, ("fine",)), ("84->64 cs=32 diff+coarse n=64", 64, 64, 32, ("diff", "coarse")),
                                   ("84->64 cs=32 coarse n=64", 64, 64, 32, ("coarse",)), ("84->64 cs=32 coarse n=128", 128, 64, 32, ("coarse",))):
        picks = torch.randint(0, a.set, (a.repeats + 5, n), generator=gen, device=dev, dtype=torch.int32)      # fresh photos every repeat
        turn = [0]

        def next_idx():
            turn[0] = (turn[0] + 1) % picks.shape[0]
            return picks[turn[0]]
        out = {f: torch.empty((n, s, s, c), device=dev) for f in fields}
        both_p = DeviceAugmenter(WINDOW).draw_device(ctx, n, PHOTO[1:])
        both_f = DeviceAugmenter((s, s)).draw_device(ctx, n, (40, 40) if s == 32 else (64, 64))
        paths = dict(warp_faces=lambda: ctx.check(lib.fg_warp_faces(h, P(photos), a.set, c, PHOTO[1], PHOTO[2], 1, P(next_idx()), P(both_p), P(both_p) + 24 * n,
                                                                    n, WINDOW[0], WINDOW[1], s, cs, P(out.get("fine")), P(out.get("coarse")),
                                                                    P(out.get("diff")), 0, 0)))
        if cs:
            paths["warp_c2f"] = lambda: ctx.check(lib.fg_warp_c2f(h, P(set64), a.set, c, 64, 64, 1, P(next_idx()), P(both_f), P(both_f) + 24 * n, n, s, cs,
                                                                  P(out.get("fine")), P(out.get("coarse")), P(out.get("diff")), 0, 0))
        else:
            paths["warp_images"] = lambda: ctx.check(lib.fg_warp_images(h, P(set40), a.set, c, 40, 40, 1, P(next_idx()), P(both_f), P(both_f) + 24 * n, n,
                                                                        P(out["fine"]), s, s, 0, 0))
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
        res[name] = {k + "_us": min_med_max(t, 1e3) for k, t in times.items()}
    return res


def bench_stages(ctx, a):
    """fg_warp_faces at n = 64 with stages left out by the choice of sizes: an 80 x 80 window copied to an 80 x 80 face is stage 1
    alone (the warp, written straight to HBM), 80 -> 32 adds stage 2 (the box mean) and writes less, 84 -> 64 without and with cs = 32
    differ by stage 3; the 32 x 32 window copied is stage 1 at the face's own size, what fg_warp_images does from LDS"""
    from face_generator_amd.runtime import DeviceAugmenter
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    gen = torch.Generator(device=dev).manual_seed(1)
    photos = photos_on_device(ctx, a.set)
    c, n = PHOTO[0], 64
    picks = torch.randint(0, a.set, (a.repeats + 5, n), generator=gen, device=dev, dtype=torch.int32)          # fresh photos every repeat
    turn = [0]

    def next_idx():
        turn[0] = (turn[0] + 1) % picks.shape[0]
        return picks[turn[0]]
    P = lambda t: None if t is None else t.data_ptr()
    cases = [("80->80 (stage 1)", 80, 80, 0), ("80->32 (stages 1, 2)", 80, 32, 0), ("32->32 (stage 1)", 32, 32, 0), ("84->32 (stages 1, 2)", 84, 32, 0),
             ("84->64 (stages 1, 2)", 84, 64, 0), ("84->64 cs=32 (stages 1, 2, 3)", 84, 64, 32)]
    calls = {}
    for name, win, s, cs in cases:
        both = DeviceAugmenter((win, win)).draw_device(ctx, n, PHOTO[1:])
        fine = torch.empty((n, s, s, c), device=dev)
        coarse = torch.empty((n, s, s, c), device=dev) if cs else None

        def call(win=win, s=s, cs=cs, both=both, fine=fine, coarse=coarse):
            ctx.check(lib.fg_warp_faces(h, P(photos), a.set, c, PHOTO[1], PHOTO[2], 1, P(next_idx()), P(both), P(both) + 24 * n, n, win, win, s, cs, P(fine),
                                        P(coarse), None, 0, 0))
        calls[name] = call
    for _ in range(5):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return dict(n=n, order="min, median, max (us)", **{k: min_med_max(t, 1e3) for k, t in times.items()})


def n_way(ctx, train, sets, B, a):
    n_epoch = 4 * B
    for data in sets.values():
        TL.timed_epoch(ctx, train, data, n_epoch)
    while any(TL.timed_epoch(ctx, train, d, n_epoch) * n_epoch < a.min_ms for d in sets.values()):
        n_epoch *= 2
    t = {k: [] for k in sets}
    for _ in range(a.rounds):
        for k, d in sets.items():
            t[k].append(TL.timed_epoch(ctx, train, d, n_epoch))
    out = dict(batch=B, N_epoch=n_epoch, rounds=a.rounds, order="min, median, max")
    for k, v in t.items():
        out[k + "_ms_per_sample"] = min_med_max(v, 1.0, 6)
        out[k + "_epoch_ms"] = min_med_max(v, n_epoch, 2)
    med = lambda k: statistics.median(t[k])
    out["photos_over_resident"] = round(med("photos") / med("resident"), 4)
    out["photos_over_device_drawn"] = round(med("photos") / med("device_drawn"), 4)
    out["device_drawn_over_resident"] = round(med("device_drawn") / med("resident"), 4)
    return out


def bench_cfg2(ctx, a):
    from face_generator_amd import models, nn_utils, adversarial
    from face_generator_amd.runtime import DeviceAugmenter, DeviceDataset, PhotoDataset
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
    sets = dict(resident=DeviceDataset(ctx, images), device_drawn=DeviceDataset(ctx, images, augment=DeviceAugmenter(dims[1:])),
                photos=PhotoDataset(ctx, photos_on_device(ctx, a.set), WINDOW, 32, augment=DeviceAugmenter(WINDOW)))
    return n_way(ctx, adversarial.train, sets, B, a)


def bench_c2f(ctx, a):
    from face_generator_amd import models_c2f, adversarial_c2f, dataset_c2f
    from face_generator_amd.runtime import DeviceAugmenter
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
    fine = torch.tensor(np.random.default_rng(2).uniform(0, 1, (a.set, 3, Sz, Sz)).astype(np.float32))
    sets = dict(resident=dataset_c2f.toResultResident(fine, Sz // 2, Sz, ctx=ctx),
                device_drawn=dataset_c2f.toResultAugmented(fine, Sz // 2, Sz, DeviceAugmenter((Sz, Sz)), ctx=ctx),
                photos=dataset_c2f.toResultPhotos(photos_on_device(ctx, a.set), WINDOW, Sz // 2, Sz, DeviceAugmenter(WINDOW), ctx=ctx))
    return n_way(ctx, adversarial_c2f.train, sets, B, a)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=("kernel", "stages", "cfg2", "c2f", "all"), default="all")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min_ms", type=float, default=300.0)
    ap.add_argument("--set", type=int, default=1024, help="photos (and face-sized images) of the synthetic sets")
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
    if a.only in ("stages", "all"):
        out["stages"] = bench_stages(ctx, a)
    if a.only in ("cfg2", "all"):
        out["cfg2_adversarial_train"] = bench_cfg2(ctx, a)
    if a.only in ("c2f", "all"):
        out["c2f_adversarial_c2f_train"] = bench_c2f(ctx, a)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
