"""Times the data pulls of one coarse-to-fine training iteration (adversarial_c2f.train: the real half's diff and coarse, the fake
half's coarse, G's coarse) three ways -- the sibling of scripts/bench_augment.py:

    (a) resident:    un-augmented gathers from the three stored sets (dataset_c2f.ResidentResult): 4 x fg_gather_images
    (b) composition: augmented with the entries of round 11: per pull fg_warp_images, then the two launches of fg_c2f_coarse_diff,
                     with a fine batch and a tmp batch through HBM: 9 launches
    (c) fused:       augmented with fg_warp_c2f, which writes only the fields a pull asks for: 3 launches

    python scripts/bench_augment_c2f.py [--repeats 30] [--inner 200] [--set 4096] [--batch 128]

A set of 3x64x64 images, coarse side 32, batch 128 (BASELINE configs 3/4), NCHW set -> NHWC batches; indices, matrices and gains
are on the device before the clock starts (what the three variants share: one draw and one upload per pull).  `inner` iterations
between two device events, the three variants alternating, `repeats` times; medians per iteration.  (b) and (c) are compared bit
for bit at the timed size.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--set", type=int, default=4096, help="images of the synthetic set")
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args(argv)
    from face_generator_amd import ops
    from face_generator_amd.runtime import get_context, Augmenter
    ctx = get_context(0)
    lib, h, dev = ctx.lib, ctx.h, ctx.device
    n_set, c, s, cs, B = a.set, 3, 64, 32, a.batch
    half = B // 2
    gen = torch.Generator(device=dev).manual_seed(1)
    fine_set = torch.rand((n_set, c, s, s), generator=gen, device=dev)
    coarse_set, diff_set = ops.c2f_coarse_diff(fine_set, cs, layout="nchw", ctx=ctx)
    P = lambda t: None if t is None else t.data_ptr()
    aug = Augmenter((s, s))
    pulls = []                              # (n, idx, mats, gains, wants diff): real half, fake half, G
    for n, want_diff in ((half, True), (half, False), (B, False)):
        mats, gains = aug.draw(n, (s, s))
        pulls.append((n, torch.randint(0, n_set, (n,), generator=gen, device=dev, dtype=torch.int32), torch.from_numpy(mats).to(dev),
                      torch.from_numpy(gains).to(dev), want_diff))
    e = c * s * s
    buf = lambda n: torch.empty(n * e, device=dev)
    out = {v: [(buf(n), buf(n)) for n, *_ in pulls] for v in "abc"}          # (coarse, diff) per pull and variant
    fine_b, tmp_b = buf(B), torch.empty(B * c * cs * cs, device=dev)

    def resident():
        for (n, idx, _, _, want_diff), (co, di) in zip(pulls, out["a"]):
            if want_diff:
                ctx.check(lib.fg_gather_images(h, P(diff_set), n_set, c, s, s, 1, P(idx), n, P(di), 0))
            ctx.check(lib.fg_gather_images(h, P(coarse_set), n_set, c, s, s, 1, P(idx), n, P(co), 0))

    def composition():
        for (n, idx, m, g, _), (co, di) in zip(pulls, out["b"]):
            ctx.check(lib.fg_warp_images(h, P(fine_set), n_set, c, s, s, 1, P(idx), P(m), P(g), n, P(fine_b), s, s, 0, 0))
            ctx.check(lib.fg_c2f_coarse_diff(h, P(fine_b), P(co), P(di), P(tmp_b), n, c, s, cs, 0))

    def fused():
        for (n, idx, m, g, want_diff), (co, di) in zip(pulls, out["c"]):
            ctx.check(lib.fg_warp_c2f(h, P(fine_set), n_set, c, s, s, 1, P(idx), P(m), P(g), n, s, cs, None, P(co), P(di) if want_diff else None, 0, 0))
    variants = dict(resident=resident, composition=composition, fused=fused)
    for _ in range(10):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner * 1e3)
    res = dict(device=torch.cuda.get_device_name(0), set=[n_set, c, s, s], coarse=cs, batch=B, pulls=[half, half, B], repeats=a.repeats, inner=a.inner,
               launches=dict(resident=4, composition=9, fused=3))
    for k, t in times.items():
        med = statistics.median(t)
        res[k + "_us_per_iteration"] = round(med, 3)
        res[k + "_us_min"] = round(min(t), 3)
        res[k + "_spread"] = round((max(t) - min(t)) / med, 4)
    res["fused_over_composition"] = round(res["fused_us_per_iteration"] / res["composition_us_per_iteration"], 4)
    res["fused_over_resident"] = round(res["fused_us_per_iteration"] / res["resident_us_per_iteration"], 4)
    # bytes through HBM per iteration as the algorithm needs them: source images read, requested fields written (+ the fine and tmp
    # batches written and read back by the composition, and the diff it has to write for every pull)
    img, small, n_all = e * 4, c * cs * cs * 4, half + half + B
    res["bytes_fused"] = n_all * img + (n_all + half) * img
    res["bytes_composition"] = n_all * (2 * img + 2 * small + 3 * img) + n_all * img
    torch.cuda.synchronize()
    same = all(torch.equal(cb.view(torch.int32), cc.view(torch.int32)) for (cb, _), (cc, _) in zip(out["b"], out["c"]))
    same = same and torch.equal(out["b"][0][1].view(torch.int32), out["c"][0][1].view(torch.int32))
    res["fused_equals_composition_bit_for_bit"] = bool(same)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
