"""sample.lua re-hosted on the sampler level of libfacegen_hip.so (runtime.Sampler: fg_sample / fg_image_grid).

Per run: 1024 images from G, D's score for each, and five pictures -- 256 random ones, all 1024, the 64 best, the 64 worst and
64 random ones -- under the file stems sample.lua:80-89 uses.  Noise, both nets, the rankings and the grids stay on the device;
every finished grid is one device-to-host copy.  With `--neighbours --trainingSet PATH` a sixth picture follows
(sample.lua:91-99): the 16 best samples, each above its nearest training image (nn_utils.findClosestNeighboursOf: the set streams
through fg_nearest_update in chunks, the samples never leave the device).  PATH is a .npy of [N][C][H][W] float32 in [0, 1] or a
directory of *.jpg / *.ppm / *.pgm files.  The commented-out c2f chain is not part of this file.

    python -m face_generator_amd.sample --save_base logs --writeto samples [--runs 1] [--batchSize 16] [--seed 1]
                                        [--neighbours --trainingSet PATH]
"""
import argparse
import glob
import os

import torch

from . import nn_utils
from .runtime import DeviceDataset, Sampler, get_context
from .state import S

N_IMAGES = 1024                      # sample.lua:80
DEFAULTS = dict(save_base="logs", G_base="adversarial.net", D_base="adversarial.net", scale=32, grayscale=False,
                writeto="samples", seed=1, gpu=0, runs=1, noiseDim=100, batchSize=16, neighbours=False, trainingSet="")
N_NEIGHBOURS = 16                    # sample.lua:94
NEIGHBOURS_STEM = "best_%04d_neighbours_base"
STEMS = ("random256_%04d_base", "random1024_%04d_base", "best_%04d_base", "worst_%04d_base", "random_%04d_base")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            ap.add_argument("--" + k, action="store_true")
        else:
            ap.add_argument("--" + k, type=type(v), default=v)
    return vars(ap.parse_args(argv))


def picture_extension():
    """.jpg through PIL when it is installed, else binary PPM / PGM written here."""
    try:
        import PIL.Image  # noqa: F401
        return ".jpg"
    except ImportError:
        return None


def output_files(opt):
    """Every file main(opt) writes, in the order it writes them."""
    ext = picture_extension() or (".pgm" if opt.get("grayscale") else ".ppm")
    stems = STEMS + ((NEIGHBOURS_STEM,) if opt.get("neighbours") else ())
    return [os.path.join(opt["writeto"], stem % run + ext) for run in range(1, opt["runs"] + 1) for stem in stems]


def save_picture(path, grid_chw):
    """image.save: a host CHW tensor with values in [0, 1] -> 8-bit picture."""
    g = (grid_chw.detach().cpu().clamp(0, 1) * 255.0 + 0.5).floor().to(torch.uint8)
    hwc = g.permute(1, 2, 0).contiguous()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if path.endswith(".jpg"):
        import PIL.Image
        arr = hwc.numpy()
        PIL.Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(path)
        return
    c, (h, w) = hwc.shape[2], hwc.shape[:2]
    if c not in (1, 3):
        raise ValueError("save_picture: %d channels (1 or 3)" % c)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if c == 1 else b"P6", w, h))
        f.write(hwc.numpy().tobytes())


def selectRandomImagesFrom(n_images, n, gen=None):
    """The first min(n, n_images) entries of a random permutation (torch.randperm) as a device int32 index tensor: which
    images go into a `random*` picture.  The images themselves stay where they are."""
    perm = torch.randperm(n_images, generator=gen)[:min(n, n_images)]
    return perm.to(torch.int32)


def toGrid(sampler, order, k, nrow):
    """image.toDisplayTensor{input = images, nrow = nrow} over images order[0..k-1] of the sampler -> host CHW tensor
    (the one copy back per picture)."""
    return sampler.grid(order, k, nrow, padding=0, normalize=True).cpu()


def loadTrainingSet(path, dims, ctx):
    """--trainingSet -> host float32 [N][C][H][W] in [0, 1] at the sampled size.  A .npy holds exactly that.  A directory is read
    as dataset.loadImages does (dataset.lua): its sorted *.jpg / *.ppm / *.pgm files, each scaled to dims with image.scale
    (ops.scale_bilinear on the device)."""
    import numpy as np
    from . import ops
    c, h, w = dims
    if not os.path.isdir(path):
        data = torch.from_numpy(np.load(path))
        if data.dtype != torch.float32 or data.dim() != 4 or tuple(data.shape[1:]) != dims:
            raise ValueError("--trainingSet %s: float32 [N][%d][%d][%d] expected, got %s %s" % (path, c, h, w, data.dtype, tuple(data.shape)))
        return data
    try:
        import PIL.Image
    except ImportError:
        raise ValueError("--trainingSet %s: reading a directory of pictures needs PIL; pass a .npy instead" % path)
    names = sorted(n for pat in ("*.jpg", "*.ppm", "*.pgm") for n in glob.glob(os.path.join(path, pat)))
    if not names:
        raise ValueError("--trainingSet %s: no *.jpg, *.ppm or *.pgm file" % path)
    out = torch.empty((len(names), c, h, w))
    for i, name in enumerate(names):
        img = np.asarray(PIL.Image.open(name).convert("L" if c == 1 else "RGB"), dtype=np.float32) / 255.0
        img = torch.from_numpy(img.reshape(img.shape[0], img.shape[1], c)).permute(2, 0, 1)[None]
        out[i] = ops.scale_bilinear(img.to(ctx.device), w, h, "nchw", ctx).cpu()[0]
    return out


def toNeighboursGrid(sampler, best, neighbours_nhwc):
    """sample.lua:156-168: sample 1, its neighbour, sample 2, ... as one picture of nrow = the number of samples, i.e. the samples
    in the upper row and each one's neighbour below it.  One device buffer [samples ; neighbours] read in the order 0, k, 1, k + 1, ..."""
    k = best.shape[0]
    both = torch.cat([best, neighbours_nhwc])
    order = torch.arange(2 * k, dtype=torch.int32).view(2, k).t().contiguous().view(-1).to(both.device)
    return sampler.grid(order, 2 * k, k, padding=0, normalize=True, images=both).cpu()


def loadModels(opt, dims):
    ck = nn_utils.load_checkpoint(os.path.join(opt["save_base"], opt["G_base"]), dims)
    G = _net_of(ck["G"], "G", dims, opt)
    if opt["D_base"] != opt["G_base"]:
        ck = nn_utils.load_checkpoint(os.path.join(opt["save_base"], opt["D_base"]), dims)
    return G, _net_of(ck["D"], "D", dims, opt)


def _net_of(entry, which, dims, opt):
    """A checkpoint holds nets (Torch7 format) or state dicts (this package's format: the net is rebuilt by MODELS)."""
    if not isinstance(entry, dict):
        return entry
    from . import models
    net = models.create_G(dims, opt["noiseDim"]) if which == "G" else models.create_D(dims)
    return nn_utils.load_state_dict(net, entry)


def main(opt=None, ctx=None):
    """-> the list of files written."""
    opt = dict(DEFAULTS, **(opt or {}))
    dims = (1 if opt["grayscale"] else 3, opt["scale"], opt["scale"])
    if opt["neighbours"] and not opt["trainingSet"]:
        raise ValueError("--neighbours needs the training set to search: pass --trainingSet PATH")
    ctx = ctx or get_context(opt["gpu"] if opt["gpu"] >= 0 else None)
    S.OPT.update(batchSize=opt["batchSize"], noiseDim=opt["noiseDim"], seed=opt["seed"], scale=opt["scale"],
                 grayscale=opt["grayscale"])
    S.IMG_DIMENSIONS = dims
    S.noise_seed, S.noise_offset = opt["seed"], 0
    gen = torch.Generator().manual_seed(opt["seed"])
    G, D = loadModels(opt, dims)
    G.cuda(ctx, opt["batchSize"])
    D.cuda(ctx, opt["batchSize"])
    S.MODEL_G, S.MODEL_D = G, D
    nn_utils.switchToEvaluationMode()
    sm = Sampler(ctx, G._inner().device_net, D._inner().device_net, N_IMAGES, opt["batchSize"])
    sm.set_seed(opt["seed"], 0)
    files = output_files(opt)
    per_run = len(STEMS) + (1 if opt["neighbours"] else 0)
    # the set goes to HBM once, in front of the run loop: every run searches it there (runtime.DeviceDataset)
    trainingSet = DeviceDataset(ctx, loadTrainingSet(opt["trainingSet"], dims, ctx)) if opt["neighbours"] else None
    print("Sampling...")
    for run in range(opt["runs"]):
        sm.sample(N_IMAGES)
        dev = lambda idx: idx.to(ctx.device)
        grids = [toGrid(sm, dev(selectRandomImagesFrom(N_IMAGES, 256, gen)), 256, 16),
                 toGrid(sm, None, N_IMAGES, 32),
                 toGrid(sm, "ORDER_DESC", 64, 8),
                 toGrid(sm, "ORDER_ASC", 64, 8),
                 toGrid(sm, dev(selectRandomImagesFrom(N_IMAGES, 64, gen)), 64, 8)]
        if opt["neighbours"]:
            best = sm.view("IMAGES").index_select(0, sm.view("ORDER_DESC")[:N_NEIGHBOURS].long())
            _, neighbours = nn_utils.findClosestNeighboursOf(best, trainingSet, ctx=ctx)
            grids.append(toNeighboursGrid(sm, best, ctx.to_device_nhwc(neighbours)))
        for path, grid in zip(files[run * per_run:], grids):
            save_picture(path, grid)
            print("wrote %s" % path)
    print("Finished.")
    return files


if __name__ == "__main__":
    main(parse_args())
