"""DATASET (coarse-to-fine): the `_toResult` step of dataset_c2f.lua:49-109 that sits directly in front of the c2f
train step: coarse = fine scaled down to coarseScale and back up to fineScale, diff = fine - coarse, wrapped as an
indexable result with .fine/.coarse/.diff.  `image.scale` runs on the device through the library's
fg_c2f_coarse_diff (csrc/image.hip scale_bilinear_kernel: the `image` package's bilinear algorithm bit for bit -- corner-aligned
linear interpolation up, fractional box mean down; the provenance note sits with the CPU restatement the parity tests use).  There is no CPU
fallback: without the library / a GPU this raises like every other compute entry.
JPEG loading (dataset_c2f.lua:111-215) is out of scope: the metric uses synthetic batches."""
import torch


class Example:
    __slots__ = ("coarse", "fine", "diff")

    def __init__(self, coarse, fine, diff):
        self.coarse, self.fine, self.diff = coarse, fine, diff


class Result:
    """dataset_c2f.lua:65-106: result.fine / .coarse / .diff tensors, result[i] -> {coarse, fine, diff}, :size()."""

    def __init__(self, fine, coarse, diff):
        self.fine, self.coarse, self.diff = fine, coarse, diff

    def size(self):
        return self.fine.shape[0]

    def __len__(self):
        return self.size()

    def getCoarse(self, index, endIndex=None):
        return self.coarse[index:endIndex] if endIndex is not None else self.coarse[index]

    def getFine(self, index, endIndex=None):
        return self.fine[index:endIndex] if endIndex is not None else self.fine[index]

    def getDiff(self, index, endIndex=None):
        return self.diff[index:endIndex] if endIndex is not None else self.diff[index]

    def __getitem__(self, i):
        return Example(self.coarse[i], self.fine[i], self.diff[i])


def toResult(fineImages, coarseScale, fineScale, ctx=None):
    """dataset._toResult (dataset_c2f.lua:49-63).  fineImages: FloatTensor [N, C, fineScale, fineScale] in [0, 1] (host, the
    reference's layout) -> Result of host tensors, computed on the device."""
    from . import ops
    from .runtime import get_context
    ctx = ctx or get_context()
    fine = torch.as_tensor(fineImages, dtype=torch.float32)
    if fine.shape[-1] != fineScale or fine.shape[-2] != fineScale:
        raise ValueError("toResult: fine images must be %dx%d" % (fineScale, fineScale))
    coarse, diff = ops.c2f_coarse_diff(fine.to(ctx.device), coarseScale, layout="nchw", ctx=ctx)
    return Result(fine.cpu(), coarse.cpu(), diff.cpu())


class ResidentResult:
    """Result with the three sets resident in HBM: .fine / .coarse / .diff are runtime.DeviceDataset objects (gather() feeds the
    c2f steps without a host round trip); size() and [i] behave as Result's do, [i] by three small copies to the host."""

    def __init__(self, fine, coarse, diff):
        self.fine, self.coarse, self.diff = fine, coarse, diff

    def size(self):
        return self.fine.size()

    def __len__(self):
        return self.size()

    def gather(self, indices, field, layout="nhwc", out=None):
        return getattr(self, field).gather(indices, layout=layout, out=out)

    def __getitem__(self, i):
        return Example(self.coarse[i], self.fine[i], self.diff[i])


def toResultResident(fineImages, coarseScale, fineScale, ctx=None, augment=None):
    """toResult that leaves the epoch's set on the device: fineImages (host or device [N, C, fineScale, fineScale]) is uploaded
    once, coarse and diff are computed once by fg_c2f_coarse_diff, and all three stay in HBM as DeviceDatasets.  An Augmenter
    (augment=, or a DeviceDataset that carries one) is refused: coarse and diff are computed once from the stored fine images, and
    a fine image under a fresh transform per batch would need both again per batch."""
    from . import ops
    from .runtime import get_context, DeviceDataset, FgError
    ctx = ctx or get_context()
    if isinstance(fineImages, DeviceDataset):
        if fineImages.storage != "f32":
            raise FgError("toResultResident: a set stored as bytes is not supported -- the stored coarse and diff fields are computed "
                          "floats; toResultAugmented computes them per batch from a byte set")
        augment = augment or fineImages.augment
        fineImages = fineImages.images
    if augment is not None:
        raise FgError("toResultResident: an augmented set is not supported -- coarse and diff are computed once from the stored "
                      "fine images; toResultAugmented computes them per batch from augmented images")
    fine = torch.as_tensor(fineImages)
    if fine.dim() != 4 or fine.shape[-1] != fineScale or fine.shape[-2] != fineScale:
        raise ValueError("toResultResident: fine images must be [N, C, %d, %d]" % (fineScale, fineScale))
    fine = DeviceDataset(ctx, fine)
    coarse, diff = ops.c2f_coarse_diff(fine.images, coarseScale, layout="nchw", ctx=ctx)
    return ResidentResult(fine, DeviceDataset(ctx, coarse), DeviceDataset(ctx, diff))


FIELDS = ("fine", "coarse", "diff")


class _PerPullResult:
    """what AugmentedResult and PhotoResult share: `set` is the resident set, gather_fields() the class's own pull; the messages
    name the class"""

    def size(self):
        return self.set.size()

    def __len__(self):
        return self.size()

    def indices(self, indices):
        """host indices (range-checked, one upload) or a device int32 tensor -> device int32 [n], as DeviceDataset.indices"""
        return self.set.indices(indices)

    def _fields(self, fields):
        from .runtime import FgError
        fields = tuple(fields)
        if not fields or len(set(fields)) != len(fields) or any(f not in FIELDS for f in fields):
            raise FgError("%s.gather_fields: fields must be a non-empty subset of %r, got %r" % (type(self).__name__, FIELDS, fields))
        return fields

    def gather(self, indices, field, layout="nhwc"):
        return self.gather_fields(indices, (field,), layout=layout)[0]

    def __getitem__(self, i):
        """Example(coarse, fine, diff) as host CHW tensors, all three under one fresh transform"""
        i = int(i)
        if i < 0 or i >= self.size():
            raise IndexError("%s: index %d outside [0, %d)" % (type(self).__name__, i, self.size()))
        coarse, fine, diff = self.gather_fields([i], ("coarse", "fine", "diff"), layout="nchw")
        return Example(coarse[0].cpu(), fine[0].cpu(), diff[0].cpu())


class AugmentedResult(_PerPullResult):
    """Result for training on freshly augmented faces: only the un-augmented fine set lives in HBM (a DeviceDataset without an
    augmenter, its images fineScale x fineScale or larger by a margin), and every pull computes the example of each picked face
    under a fresh random transform: warp to fineScale, scale down to coarseScale and back up, subtract, in one launch of
    fg_warp_c2f.  gather_fields() hands out several fields of the SAME transforms (the real half of a D iteration needs diff and
    coarse of one warped face); gather() is the one-field form, so the loops that feed a ResidentResult feed this class too."""

    def __init__(self, fine, coarseScale, fineScale, augment):
        from .runtime import Augmenter, DeviceDataset, FgError
        if not isinstance(fine, DeviceDataset) or fine.augment is not None:
            raise FgError("AugmentedResult: the set must be a DeviceDataset without an augmenter (the result holds the augmenter)")
        if not isinstance(augment, Augmenter):
            raise FgError("AugmentedResult: augment must be a runtime.Augmenter")
        self.coarseScale, self.fineScale = int(coarseScale), int(fineScale)
        if tuple(augment.out_hw) != (self.fineScale, self.fineScale):
            raise FgError("AugmentedResult: the augmenter hands out %dx%d images, the fine scale is %d" % (augment.out_hw + (self.fineScale,)))
        if not 1 <= self.coarseScale <= self.fineScale:
            raise FgError("AugmentedResult: coarse scale %d outside 1 .. %d" % (self.coarseScale, self.fineScale))
        self.set, self.augment, self.ctx = fine, augment, fine.ctx

    def gather_fields(self, indices, fields, layout="nhwc"):
        """-> a tuple of device tensors [n][S][S][C] ("nhwc") or [n][C][S][S] ("nchw") in the order of `fields`, a subset of
        ("fine", "coarse", "diff"): field f of dataset[indices[j]] under transform j.  One Augmenter.draw of n transforms shared
        by all fields, one upload, one launch; a runtime.DeviceAugmenter draws on the device instead (fg_draw_transforms: no
        host draw, no upload)."""
        from . import ops
        from .runtime import FgError
        if layout not in ("nhwc", "nchw"):
            raise FgError("AugmentedResult.gather_fields: layout must be 'nhwc' or 'nchw'")
        fields = self._fields(fields)
        idx = self.indices(indices)
        n, ds, s = int(idx.numel()), self.set, self.fineScale
        if not n:
            shape = (0, s, s, ds.c) if layout == "nhwc" else (0, ds.c, s, s)
            return tuple(self.ctx.empty(*shape) for _ in fields)
        both = self.augment.draw_device(self.ctx, n, (ds.h, ds.w))
        return ops.warp_c2f(ds.images, idx, s, self.coarseScale, mats=both[:6 * n], gains=both[6 * n:], fields=fields, set_layout="nchw",
                            out_layout=layout, fill=self.augment.fill, ctx=self.ctx, gray=ds.gray and ds.storage == "u8")


def toResultAugmented(fineImages, coarseScale, fineScale, augment, ctx=None, storage="f32", gray=False):
    """toResult for training on freshly augmented faces: fineImages (host or device [N, C, H, W] with H, W >= fineScale, or a
    DeviceDataset without an augmenter) is uploaded once and stays un-augmented in HBM; `augment`, an Augmenter whose out_hw is
    (fineScale, fineScale), draws the transforms of every pull -> AugmentedResult.  storage: DeviceDataset's ("u8": uint8 images
    stay bytes in HBM, pixels of value b / 255) and gray (images of 3 channels, examples of their luma: one channel; with "u8"
    every pull is one launch of fg_warp_c2f_u8_y on the R, G, B bytes); a DeviceDataset keeps its own."""
    from .runtime import get_context, DeviceDataset, FgError
    ctx = ctx or get_context()
    if not isinstance(fineImages, DeviceDataset):
        fine = torch.as_tensor(fineImages)
        if fine.dim() != 4 or fine.shape[-1] < fineScale or fine.shape[-2] < fineScale:
            raise ValueError("toResultAugmented: fine images must be [N, C, H, W] with H, W >= %d" % fineScale)
        fineImages = DeviceDataset(ctx, fine, storage=storage, gray=gray)
    elif fineImages.augment is not None:
        raise FgError("toResultAugmented: hand the Augmenter over as augment=, not on the DeviceDataset")
    return AugmentedResult(fineImages, coarseScale, fineScale, augment)


class PhotoResult(_PerPullResult):
    """AugmentedResult for a set of whole photos (runtime.PhotoDataset, which holds the augmenter): every pull warps the picked
    photos in photo coordinates into the face window, scales the window to fineScale with image.scale and computes coarse and diff
    from that face, in one launch of fg_warp_faces.  The interface is AugmentedResult's: size, indices, gather_fields, gather,
    [i] -> Example."""

    def __init__(self, photos, coarseScale):
        from .runtime import PhotoDataset, FgError
        if not isinstance(photos, PhotoDataset):
            raise FgError("PhotoResult: the set must be a runtime.PhotoDataset")
        self.coarseScale, self.fineScale = int(coarseScale), photos.h
        if not 1 <= self.coarseScale <= self.fineScale:
            raise FgError("PhotoResult: coarse scale %d outside 1 .. %d" % (self.coarseScale, self.fineScale))
        self.set, self.ctx = photos, photos.ctx

    @property
    def augment(self):
        return self.set.augment

    def gather_fields(self, indices, fields, layout="nhwc"):
        """-> a tuple of device tensors [n][S][S][C] ("nhwc") or [n][C][S][S] ("nchw") in the order of `fields`, a subset of
        ("fine", "coarse", "diff"): field f of the face of photo indices[j] under transform j.  One draw shared by all fields,
        one launch."""
        return self.set.gather_fields(indices, self._fields(fields), coarse_scale=self.coarseScale, layout=layout)


def toResultPhotos(photos, window_hw, coarseScale, fineScale, augment, ctx=None, storage="f32", gray=False):
    """toResult for training on faces cut from whole photos under fresh transforms: photos (host or device [N, C, H, W], any H and
    W, or a runtime.PhotoDataset, which then carries window, fine scale and augmenter itself) is uploaded once and stays in HBM;
    `augment`, an Augmenter whose out_hw is window_hw (or None: the central window, un-augmented), draws the transforms of every
    pull -> PhotoResult.  storage: PhotoDataset's ("u8": uint8 photos stay bytes in HBM, pixels of value b / 255) and gray (photos
    of 3 channels, examples of their luma: one channel; with "u8" every pull is one launch of fg_warp_faces_u8_y); a PhotoDataset
    keeps its own."""
    from .runtime import get_context, PhotoDataset, FgError
    if isinstance(photos, PhotoDataset):
        if augment is not None and augment is not photos.augment:
            raise FgError("toResultPhotos: the PhotoDataset carries its own augmenter")
        if photos.h != int(fineScale) or photos.window_hw != tuple(window_hw if not isinstance(window_hw, int) else (window_hw, window_hw)):
            raise FgError("toResultPhotos: the PhotoDataset hands out %dx%d faces of a %dx%d window" % ((photos.h, photos.w) + photos.window_hw))
        return PhotoResult(photos, coarseScale)
    return PhotoResult(PhotoDataset(ctx or get_context(), photos, window_hw, int(fineScale), augment=augment, storage=storage, gray=gray),
                       coarseScale)


def toResultDevice(fine_nhwc, coarseScale, ctx=None):
    """The same step for a batch that already lives in HBM in the library's activation layout [N][S][S][C]: -> (coarse, diff) device
    tensors, the inputs of TrainerC2F.step_D / step_G."""
    from . import ops
    return ops.c2f_coarse_diff(fine_nhwc, coarseScale, layout="nhwc", ctx=ctx)
