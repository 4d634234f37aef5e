"""MODELS: the reference's model zoo for the hot path (models.lua), as layer lists for fg_net_create.

Same public names as models.lua: `create_G(dimensions, noiseDim)` (models.lua:87-93 -> create_G_decoder_upsampling32,
:57-81) and `create_D(dimensions)` (models.lua:98-104 -> create_D32b, :382-416).  Each returns an `nn.Sequential`
(face_generator_amd.nn) whose modules mirror the Torch7 modules one for one.
"""
from . import nn
from .nn import cudnn
from .weight_init import w_init


def create_G_decoder_upsampling32(dimensions, noiseDim, gen=None):
    """models.lua:57-81."""
    model = nn.Sequential()
    model.add(nn.Linear(noiseDim, 128 * 8 * 8))
    model.add(nn.View(128, 8, 8))
    model.add(nn.PReLU())

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(128, 256, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(nn.PReLU())

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(256, 128, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(nn.PReLU())

    model.add(cudnn.SpatialConvolution(128, dimensions[0], 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.Sigmoid())
    model.input_dims = (noiseDim, 1, 1)
    model = w_init(model, 'heuristic', gen=gen)      # models.lua:48 / :78
    return model


def create_G_decoder_upsampling16(dimensions, noiseDim, gen=None):
    """models.lua:27-51: the same decoder started from a 4x4 map (no new kernel class)."""
    model = nn.Sequential()
    model.add(nn.Linear(noiseDim, 128 * 4 * 4))
    model.add(nn.View(128, 4, 4))
    model.add(nn.PReLU())

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(128, 256, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(nn.PReLU())

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(256, 128, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(nn.PReLU())

    model.add(cudnn.SpatialConvolution(128, dimensions[0], 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.Sigmoid())
    model.input_dims = (noiseDim, 1, 1)
    model = w_init(model, 'heuristic', gen=gen)      # models.lua:48 / :78
    return model


def create_G(dimensions, noiseDim, gen=None):
    """models.lua:87-93."""
    if dimensions[1] == 16:
        return create_G_decoder_upsampling16(dimensions, noiseDim, gen=gen)
    return create_G_decoder_upsampling32(dimensions, noiseDim, gen=gen)


def create_D32b(dimensions):
    """models.lua:382-416."""
    conv = nn.Sequential()
    c, h, w = dimensions
    for (i, o) in ((c, 64), (64, 128), (128, 256), (256, 512)):
        conv.add(nn.SpatialConvolution(i, o, 3, 3, 1, 1, (3 - 1) // 2))
        conv.add(nn.PReLU())
        conv.add(nn.SpatialDropout(0.2))
        conv.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    nfeat = int(512 * 0.25 * 0.25 * 0.25 * 0.25 * h * w)
    conv.add(nn.View(nfeat))
    conv.add(nn.Linear(nfeat, 512))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout())
    conv.add(nn.Linear(512, 512))
    conv.add(nn.PReLU())
    conv.add(nn.Dropout())
    conv.add(nn.Linear(512, 1))
    conv.add(nn.Sigmoid())
    conv.input_dims = (c, h, w)
    return conv


def create_D16_d(dimensions):
    """models.lua:279-316: ConcatTable{conv branch with two stride-2 convs, dense branch} -> JoinTable(2) -> Linear -> Sigmoid
    (SURVEY 8(f) rank 4)."""
    c, h, w = dimensions
    inputSz = c * h * w
    fine = nn.Sequential()
    fine.add(nn.SpatialConvolution(c, 128, 3, 3, 1, 1, (3 - 1) // 2))
    fine.add(nn.PReLU())
    fine.add(nn.SpatialConvolution(128, 128, 3, 3, 1, 1, (3 - 1) // 2))
    fine.add(nn.PReLU())
    fine.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    fine.add(nn.SpatialConvolution(128, 512, 3, 3, 2, 2, (3 - 1) // 2))
    fine.add(nn.PReLU())
    fine.add(nn.SpatialConvolution(512, 1024, 3, 3, 2, 2, (3 - 1) // 2))
    fine.add(nn.PReLU())
    fine.add(nn.SpatialDropout())
    fine_size = int(1024 * 0.25 * 0.25 * 0.25 * h * w)
    fine.add(nn.View(fine_size))
    fine.add(nn.Linear(fine_size, 1024))
    fine.add(nn.PReLU())

    dense = nn.Sequential()
    dense.add(nn.View(inputSz))
    dense.add(nn.Linear(inputSz, 128))
    dense.add(nn.PReLU())
    dense.add(nn.Dropout())
    dense.add(nn.Linear(128, 128))
    dense.add(nn.PReLU())

    tail = nn.Sequential()
    tail.add(nn.Linear(1024 + 128, 1))
    tail.add(nn.Sigmoid())
    model = nn.ConcatSequential([fine, dense], tail)
    model.input_dims = (c, h, w)
    return model


def _seq(mods, dimensions):
    s = nn.Sequential()
    for m in mods:
        s.add(m)
    s.input_dims = tuple(dimensions)
    return s


def _conv(i, o, k, stride=1):
    return nn.SpatialConvolution(i, o, k, k, stride, stride, (k - 1) // 2)


def _dense_branch(inputSz, dimensions):
    """The dense branch every three-branch discriminator shares (models.lua:138-144, 192-198, 250-256, 352-358)."""
    return _seq([nn.View(inputSz), nn.Linear(inputSz, 1024), nn.PReLU(), nn.Dropout(), nn.Linear(1024, 1024), nn.PReLU()], dimensions)


def _table_D(branches, joined, dimensions):
    """ConcatTable{branches} -> JoinTable(2) -> Linear(joined, 1024) -> PReLU -> Dropout -> Linear(1024, 1) -> Sigmoid
    (models.lua:146-160, 200-214, 258-272, 360-374)."""
    tail = _seq([nn.Linear(joined, 1024), nn.PReLU(), nn.Dropout(), nn.Linear(1024, 1), nn.Sigmoid()], (joined, 1, 1))
    model = nn.ConcatSequential(branches, tail)
    model.input_dims = tuple(dimensions)
    return model


def create_D16(dimensions):
    """models.lua:110-160 create_D16: ConcatTable{fine 3x3 branch, coarse 5x5 branch, dense branch}, each conv branch
    conv-PReLU-conv-PReLU-MaxPool(2,2)-SpatialDropout(0.5)-View-Linear(.., 1024)-PReLU-Dropout(0.5)."""
    c, h, w = dimensions
    flat = 64 * h * w // 4
    fine = _seq([_conv(c, 64, 3), nn.PReLU(), _conv(64, 64, 3), nn.PReLU(), nn.SpatialMaxPooling(2, 2), nn.SpatialDropout(),
                 nn.View(flat), nn.Linear(flat, 1024), nn.PReLU(), nn.Dropout()], dimensions)
    coarse = _seq([_conv(c, 32, 5), nn.PReLU(), _conv(32, 64, 5), nn.PReLU(), nn.SpatialMaxPooling(2, 2), nn.SpatialDropout(),
                   nn.View(flat), nn.Linear(flat, 1024), nn.PReLU(), nn.Dropout()], dimensions)
    return _table_D([fine, coarse, _dense_branch(c * h * w, dimensions)], 1024 + 1024 + 1024, dimensions)


def _strided_branch(c, k, widths_strides, flat, nout, dropout, dimensions):
    mods, i = [], c
    for o, stride in widths_strides:
        mods += [_conv(i, o, k, stride), nn.PReLU()]
        i = o
    mods += [nn.SpatialDropout(), nn.View(flat), nn.Linear(flat, nout), nn.PReLU()]
    if dropout:
        mods.append(nn.Dropout())
    return _seq(mods, dimensions)


def create_D16_b(dimensions):
    """models.lua:161-216 create_D16_b: a 3x3 and a 5x5 branch of convolutions c-64-64-128-128, the last with stride 2, then
    SpatialDropout(0.5)-View-Linear(.., 512)-PReLU-Dropout(0.5); the dense branch; Linear(512 + 512 + 1024, 1024) behind the join."""
    c, h, w = dimensions
    flat = 128 * h * w // 4
    ws = [(64, 1), (64, 1), (128, 1), (128, 2)]
    return _table_D([_strided_branch(c, 3, ws, flat, 512, True, dimensions), _strided_branch(c, 5, ws, flat, 512, True, dimensions),
                     _dense_branch(c * h * w, dimensions)], 512 + 512 + 1024, dimensions)


def create_D16_c(dimensions):
    """models.lua:218-274 create_D16_c: the branches of create_D16_b with a fifth convolution 128 -> 512 at stride 2, Linear(.., 1024)
    and no Dropout at the end of the two conv branches."""
    c, h, w = dimensions
    flat = 512 * h * w // 16
    ws = [(64, 1), (64, 1), (128, 1), (128, 2), (512, 2)]
    return _table_D([_strided_branch(c, 3, ws, flat, 1024, False, dimensions), _strided_branch(c, 5, ws, flat, 1024, False, dimensions),
                     _dense_branch(c * h * w, dimensions)], 1024 + 1024 + 1024, dimensions)


def create_D32(dimensions):
    """models.lua:322-376 create_D32.  The Lua function reads the globals IMG_DIMENSIONS / INPUT_SZ (train.lua:84-91) instead of its
    argument; they are the image dimensions, taken from `dimensions` here.  Fine branch: 3x3 c-64-64, MaxPool(2,2),
    SpatialDropout(0.5), Linear(.., 1024), PReLU.  Coarse branch: 5x5 c-32-32, MaxPool, 5x5 32-54-54, MaxPool, SpatialDropout(0.5),
    Linear(.., 1024)-PReLU-Dropout(0.5)-Linear(1024, 1024)-PReLU."""
    c, h, w = dimensions
    flat_f, flat_c = 64 * h * w // 4, 54 * h * w // 16
    fine = _seq([_conv(c, 64, 3), nn.PReLU(), _conv(64, 64, 3), nn.PReLU(), nn.SpatialMaxPooling(2, 2), nn.SpatialDropout(),
                 nn.View(flat_f), nn.Linear(flat_f, 1024), nn.PReLU()], dimensions)
    coarse = _seq([_conv(c, 32, 5), nn.PReLU(), _conv(32, 32, 5), nn.PReLU(), nn.SpatialMaxPooling(2, 2),
                   _conv(32, 54, 5), nn.PReLU(), _conv(54, 54, 5), nn.PReLU(), nn.SpatialMaxPooling(2, 2), nn.SpatialDropout(),
                   nn.View(flat_c), nn.Linear(flat_c, 1024), nn.PReLU(), nn.Dropout(), nn.Linear(1024, 1024), nn.PReLU()], dimensions)
    return _table_D([fine, coarse, _dense_branch(c * h * w, dimensions)], 1024 + 1024 + 1024, dimensions)


def create_D(dimensions):
    """models.lua:98-104."""
    if dimensions[1] == 16:
        return create_D16_d(dimensions)
    return create_D32b(dimensions)
