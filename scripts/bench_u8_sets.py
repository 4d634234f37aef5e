"""Times the three warps on a set held as 8-bit pixels (fg_warp_images_u8, fg_warp_c2f_u8, fg_warp_faces_u8) beside their fp32
siblings, and what the byte storage saves -- the sibling of scripts/bench_augment_photos.py, whose sizes and helpers it uses.

    python scripts/bench_u8_sets.py [--set 1024] [--repeats 50]

Kernel: per entry, at the pull sizes of scripts/bench_augment_photos.py (84 -> 32 without fields and 40 -> 32 at n = 64; 84 -> 64 and
64 -> 64 with cs = 32 for ("diff", "coarse") at n = 64 and for ("coarse",) at n = 64 and n = 128), the fp32 and the u8 instance
alternating in one process on a set of random bytes and on the float set b / 255, the same transforms, fresh random indices every
repeat, device events around each repeat, min / median / max.  Storage: the bytes of HBM a set of --set photos of 250 x 250 x 3 holds
as a runtime.PhotoDataset in both storages, and the time from the host array to the set in HBM (conversion and upload, synchronised),
min / median / max of five.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment_photos import PHOTO, WINDOW, min_med_max  # noqa: E402  (puts the package on the path too)


def decode(b):
    # the correctly rounded quotient, as the header states the value of a byte (a tensor divisor: a true division per element)
    return b.to(torch.float32) / torch.full((), 255.0, device=b.device)


def bench_kernel(ctx, a):
    from face_generator_amd.runtime import DeviceAugmenter
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    gen = torch.Generator(device=dev).manual_seed(1)
    c = PHOTO[0]
    bytes_of = lambda hw: torch.randint(0, 256, (a.set, c) + hw, generator=gen, device=dev, dtype=torch.uint8)
    sets8 = dict(photos=bytes_of(PHOTO[1:]), set40=bytes_of((40, 40)), set64=bytes_of((64, 64)))
    sets32 = {k: decode(v) for k, v in sets8.items()}
    P = lambda t: None if t is None else t.data_ptr()
    res = dict(n_set=a.set, photo=list(PHOTO), window=list(WINDOW), repeats=a.repeats, order="min, median, max (us)")
    for name, n, s, cs, fields in (("84->32 fine n=64", 64, 32, 0, ("fine",)), ("84->64 cs=32 diff+coarse n=64", 64, 64, 32, ("diff", "coarse")),
                                   ("84->64 cs=32 coarse n=64", 64, 64, 32, ("coarse",)), ("84->64 cs=32 coarse n=128", 128, 64, 32, ("coarse",))):
        picks = torch.randint(0, a.set, (a.repeats + 5, n), generator=gen, device=dev, dtype=torch.int32)      # fresh images every repeat
        turn = [0]

        def next_idx():
            turn[0] = (turn[0] + 1) % picks.shape[0]
            return picks[turn[0]]
        out = {f: torch.empty((n, s, s, c), device=dev) for f in fields}
        both_p = DeviceAugmenter(WINDOW).draw_device(ctx, n, PHOTO[1:])
        both_f = DeviceAugmenter((s, s)).draw_device(ctx, n, (40, 40) if s == 32 else (64, 64))
        O = lambda f: P(out.get(f))
        paths = {}
        for tag, sets, suffix in (("f32", sets32, ""), ("u8", sets8, "_u8")):
            def faces(sets=sets, fn=getattr(lib, "fg_warp_faces" + suffix)):
                ctx.check(fn(h, P(sets["photos"]), a.set, c, PHOTO[1], PHOTO[2], 1, P(next_idx()), P(both_p), P(both_p) + 24 * n, n, WINDOW[0], WINDOW[1],
                             s, cs, O("fine"), O("coarse"), O("diff"), 0, 0))

            def c2f(sets=sets, fn=getattr(lib, "fg_warp_c2f" + suffix)):
                ctx.check(fn(h, P(sets["set64"]), a.set, c, 64, 64, 1, P(next_idx()), P(both_f), P(both_f) + 24 * n, n, s, cs, O("fine"), O("coarse"),
                             O("diff"), 0, 0))

            def images(sets=sets, fn=getattr(lib, "fg_warp_images" + suffix)):
                ctx.check(fn(h, P(sets["set40"]), a.set, c, 40, 40, 1, P(next_idx()), P(both_f), P(both_f) + 24 * n, n, O("fine"), s, s, 0, 0))
            paths["warp_faces_" + tag] = faces
            paths["warp_c2f_" + tag if cs else "warp_images_" + tag] = c2f if cs else images
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
    for tag, host, kw in (("f32", host32, {}), ("u8", host8, dict(storage="u8"))):
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
