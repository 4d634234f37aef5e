"""Times the three warps on a set of R, G, B bytes read as luma (fg_warp_images_u8_y, fg_warp_c2f_u8_y, fg_warp_faces_u8_y) beside
(a) their _u8 siblings on the same bytes, three channels out: the same reads, a third of the arithmetic and of the writes, and (b)
their fp32 siblings on the pre-converted one-channel float set: what a grayscale run has to do without them -- the sibling of
scripts/bench_u8_sets.py.

    python scripts/bench_gray_sets.py [--set 1024] [--repeats 50]

Kernel: 64 faces per pull at the workload's sizes -- 64 x 64 -> 32 x 32 images, 64 -> 64 / 32 c2f ("diff", "coarse"), 250 x 250
photos through the 84 window to 32 ("fine") and to 64 / 32 ("diff", "coarse") -- the instances alternating in one process on a
set of random bytes (the luma entry on its planes, "y", and on the same pixels as triples, "y_pm") and on its float luma, the same
transforms, fresh random indices every repeat, device events around each repeat, min / median / max.  Storage: the bytes of HBM a set of --set photos of 3 x 250 x 250 holds as a gray runtime.PhotoDataset in both
storages, and the time from the host array to the set in HBM (conversion and upload, synchronised), min / median / max of five.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment_photos import PHOTO, WINDOW, min_med_max  # noqa: E402  (puts the package on the path too)


def bench_kernel(ctx, a):
    from face_generator_amd.runtime import DeviceAugmenter, _luma_f32
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    gen = torch.Generator(device=dev).manual_seed(1)
    n = 64
    bytes_of = lambda hw: torch.randint(0, 256, (a.set, 3) + hw, generator=gen, device=dev, dtype=torch.uint8)
    sets8 = dict(photos=bytes_of(PHOTO[1:]), set64=bytes_of((64, 64)))
    sets8pm = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in sets8.items()}     # the same pixels, R, G, B adjacent
    # the one-channel float sets: Y of the floats b / 255 (a tensor divisor: a true division per element)
    sets32 = {k: _luma_f32(ctx, v.to(torch.float32) / torch.full((), 255.0, device=dev)) for k, v in sets8.items()}
    P = lambda t: None if t is None else t.data_ptr()
    res = dict(n_set=a.set, n=n, photo=list(PHOTO), window=list(WINDOW), repeats=a.repeats, order="min, median, max (us)")
    for name, entry, s, cs, fields in (("images 64->32 fine", "images", 32, 0, ("fine",)), ("c2f 64->64/32 diff+coarse", "c2f", 64, 32, ("diff", "coarse")),
                                       ("faces 250->84->32 fine", "faces", 32, 0, ("fine",)),
                                       ("faces 250->84->64/32 diff+coarse", "faces", 64, 32, ("diff", "coarse"))):
        picks = torch.randint(0, a.set, (a.repeats + 5, n), generator=gen, device=dev, dtype=torch.int32)      # fresh images every repeat
        turn = [0]

        def next_idx():
            turn[0] = (turn[0] + 1) % picks.shape[0]
            return picks[turn[0]]
        out = {f: torch.empty((n, s, s, 3), device=dev) for f in fields}       # (the one-channel calls write the first third)
        both = DeviceAugmenter(WINDOW).draw_device(ctx, n, PHOTO[1:]) if entry == "faces" else DeviceAugmenter((s, s)).draw_device(ctx, n, (64, 64))
        O = lambda f: P(out.get(f))
        m, g = P(both), P(both) + 24 * n

        def call(tag):
            # "y" / "y_pm": the luma entry on the planes / the triples; "u8": the byte entry on the planes, three channels; "f32":
            # the fp32 entry at c = 1
            src = sets32 if tag == "f32" else sets8pm if tag == "y_pm" else sets8
            fn = getattr(lib, "fg_warp_" + entry + dict(y="_u8_y", y_pm="_u8_y", u8="_u8", f32="")[tag])
            c = () if tag in ("y", "y_pm") else (3,) if tag == "u8" else (1,)
            ol = () if tag in ("y", "y_pm") else (0,)
            sl = 0 if tag == "y_pm" else 1
            if entry == "images":
                return lambda: ctx.check(fn(h, P(src["set64"]), a.set, *c, 64, 64, sl, P(next_idx()), m, g, n, O("fine"), s, s, *ol, 0))
            if entry == "c2f":
                return lambda: ctx.check(fn(h, P(src["set64"]), a.set, *c, 64, 64, sl, P(next_idx()), m, g, n, s, cs, O("fine"), O("coarse"), O("diff"), *ol, 0))
            return lambda: ctx.check(fn(h, P(src["photos"]), a.set, *c, PHOTO[1], PHOTO[2], sl, P(next_idx()), m, g, n, WINDOW[0], WINDOW[1], s, cs, O("fine"),
                                        O("coarse"), O("diff"), *ol, 0))
        paths = {"warp_%s_%s" % (entry, tag): call(tag) for tag in ("y", "y_pm", "u8", "f32")}
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
        res[name] = {k + "_us": min_med_max(t, 1e3) for k, t in sorted(times.items())}
    return res


def bench_storage(ctx, a):
    from face_generator_amd.runtime import PhotoDataset
    host8 = np.random.default_rng(3).integers(0, 256, (a.set,) + PHOTO, dtype=np.uint8)
    host32 = host8.astype(np.float32) / np.float32(255)             # what a host loader hands over today
    res = dict(n_photos=a.set, photo=list(PHOTO), order="min, median, max (ms)")
    for tag, host, kw in (("f32_gray", host32, dict(gray=True)), ("u8_gray", host8, dict(storage="u8", gray=True))):
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = PhotoDataset(ctx, host, WINDOW, 32, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res[tag + "_hbm_bytes"] = ds.photos.numel() * ds.photos.element_size()
        res[tag + "_host_bytes"] = int(host.nbytes)
        res[tag + "_upload_ms"] = min_med_max(times, 1e3)
        del ds
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--set", type=int, default=1024, help="images of the synthetic sets")
    ap.add_argument("--repeats", type=int, default=50)
    a = ap.parse_args(argv)
    from face_generator_amd.runtime import get_context
    ctx = get_context(0)
    out = dict(device=torch.cuda.get_device_name(0), kernel=bench_kernel(ctx, a), storage=bench_storage(ctx, a))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
