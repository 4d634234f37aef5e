"""Small nets off the models' shapes, one per decision of the net planner (fg_net_create, forward_run and the backward walk of
csrc/net.hip): the grammar of layer lists, the fixed NET_CASES, and the two builders that make the oracle.torch7_nn module tree and
the DeviceNet from one list.  Module-level data and helpers, no GPU use at import: tests/dispatch_audit.py runs the lists in the
planning-only context (net_sweep, net_replay), tests/test_net_fusions_host.py asserts on the logs, tests/test_gpu_net_fusions.py
compares every case with the float64 oracle.  tests/NET_FUSIONS.md is the table of decisions with the case names.

A layer is the tuple runtime.make_specs takes: (TYPE, a, b, c, d, p, q), short ones padded with zeros."""
import collections
import ctypes
import zlib

import numpy as np

FUSIONS = (503, 23, 502)      # the default; the Winograd bits cleared (implicit GEMM everywhere); FG_FUSE_PRELU cleared
MATHS = (0, 6)
MARKERS = ("CONCAT_TABLE", "BRANCH", "JOIN_TABLE")
IN_C = [1, 2, 3, 4, 8, 16, 64]
CHANNELS = [1, 2, 3, 4, 5, 6, 8, 12, 16, 32, 64, 128]
LINEAR_OUT = [1, 2, 5, 7, 10, 16, 48, 64, 100, 128]
SWEEP_SEED, SWEEP_N = 20261019, 2000


def pad(l):
    return tuple(l) + (0,) * (7 - len(l))


# ---------------------------------------------------------------------------------------------------------------------------------
# shapes: what every layer of a list produces, on the oracle's side (NCHW, Torch7) and on the device's (NHWC; behind a flatten the
# features keep the NHWC order of the map until a Linear consumes them -- `perm` is that map's (C, H, W))
# ---------------------------------------------------------------------------------------------------------------------------------
Out = collections.namedtuple("Out", "shape chw perm")       # oracle shape without the batch; device (c, h, w); pending (C, H, W)


def walk(layers, dims):
    """-> (input Out, [Out per layer]); a marker's entry is the state behind it (BRANCH: the net's input, JOIN_TABLE: the joined row).
    Raises ValueError for a list that is not valid Torch7 (a size mismatch)."""
    c, h, w = dims
    flat = h * w == 1              # a vector input: Torch7 sees [B][F]
    first = Out((c,) if flat else (c, h, w), (c, h, w), None)
    cur, outs, widths = first, [], []
    for l in layers:
        t, a, b, cc, d, p, q = pad(l)
        c, h, w = cur.chw
        isflat = len(cur.shape) == 1
        if t == "CONCAT_TABLE":
            widths = []
        elif t == "BRANCH":
            if outs and layers[len(outs) - 1][0] != "CONCAT_TABLE":
                widths.append(cur.chw[0])
            cur = first
        elif t == "JOIN_TABLE":
            widths.append(cur.chw[0])
            cur = Out((sum(widths),), (sum(widths), 1, 1), None)
        elif t == "LINEAR":
            if not isflat or a != c:
                raise ValueError("Linear input %d on %s" % (a, cur.shape))
            cur = Out((b,), (b, 1, 1), None)
        elif t == "VIEW":
            if b > 0:
                if a * b * cc != c * h * w:
                    raise ValueError("View size")
                cur = Out((a, b, cc), (a, b, cc), None)
            else:
                if a != c * h * w:
                    raise ValueError("View size")
                cur = Out((a,), (a, 1, 1), cur.perm if isflat else ((c, h, w) if h * w > 1 else None))
        elif isflat and t in ("CONV", "UPSAMPLE2X", "BATCHNORM", "SPATIAL_DROPOUT", "AVGPOOL2", "MAXPOOL2"):
            raise ValueError("%s on a vector" % t)
        elif t == "CONV":
            if a != c:
                raise ValueError("conv nInputPlane")
            s, f = (2 if p == 2 else 1), (int(q) if q > 1 else 1)
            if s == 2 and (h % 2 or w % 2):
                raise ValueError("stride 2 on an odd map")        # ('same' pad: Torch7 would floor; the header rules it out)
            cur = Out((b // (f * f), h // s * f, w // s * f), (b // (f * f), h // s * f, w // s * f), None)
        elif t == "UPSAMPLE2X":
            cur = Out((c, 2 * h, 2 * w), (c, 2 * h, 2 * w), None)
        elif t in ("AVGPOOL2", "MAXPOOL2"):
            if h % 2 or w % 2:
                raise ValueError("pool on an odd map")
            cur = Out((c, h // 2, w // 2), (c, h // 2, w // 2), None)
        elif t == "BATCHNORM" and a != c:
            raise ValueError("BatchNorm nFeature")
        outs.append(cur)
    return first, outs


def to_device(a, out):
    """oracle array [B] + out.shape -> the device's layout as a numpy array ([B][H][W][C], or [B][F] in the pending NHWC order)"""
    B = a.shape[0]
    if out.perm is not None:
        C, H, W = out.perm
        return np.ascontiguousarray(a.reshape(B, C, H, W).transpose(0, 2, 3, 1)).reshape(B, -1)
    if len(out.shape) == 3:
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    return np.ascontiguousarray(a)


def from_device(a, out):
    """the reverse: a device array of any shape with B rows -> [B] + out.shape"""
    B = a.shape[0]
    if out.perm is not None:
        C, H, W = out.perm
        return a.reshape(B, H, W, C).transpose(0, 3, 1, 2).reshape((B,) + out.shape)
    if len(out.shape) == 3:
        C, H, W = out.shape
        return a.reshape(B, H, W, C).transpose(0, 3, 1, 2)
    return a.reshape((B,) + out.shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# the grammar
# ---------------------------------------------------------------------------------------------------------------------------------
def _spatial_run(r, c, h, w, n, in_branch=False):
    """n draws of layers on a [c][h][w] map; -> (layers, c, h, w)"""
    L = []
    pick = lambda xs: xs[int(r.integers(len(xs)))]
    for _ in range(n):
        t = pick(["CONV", "CONV", "CONV", "UPCONV", "PRELU", "PRELU", "ACTPOOL", "ACTMAXPOOL", "BATCHNORM", "BNPRELU", "SPATIAL_DROPOUT",
                  "AVGPOOL2", "MAXPOOL2", "UPSAMPLE2X", "LEAKYRELU", "DROPOUT", "SIGMOID", "CONVSIG"])
        if t in ("CONV", "UPCONV", "CONVSIG"):
            if t == "UPCONV":
                if h * w > 64:
                    continue
                L.append(("UPSAMPLE2X",)); h *= 2; w *= 2
            k = pick([3, 3, 5, 7])
            co = pick([1, 2, 3]) if t == "CONVSIG" else pick(CHANNELS)
            st = 2 if (r.random() < 0.2 and h % 2 == 0 and w % 2 == 0) else 0
            f = 2 if (st == 0 and r.random() < 0.12 and h * w <= 64) else 0        # the SpatialConvolutionUpsample factor
            L.append(("CONV", c, co * (f * f if f else 1), k, (k - 1) // 2, st, f))
            c = co
            if st == 2:
                h //= 2; w //= 2
            if f:
                h *= f; w *= f
            if t == "CONVSIG":
                L.append(("SIGMOID",))
        elif t in ("BATCHNORM", "BNPRELU"):
            if c % 4 or in_branch:
                continue
            L.append(("BATCHNORM", c))
            if t == "BNPRELU":
                L.append(("PRELU",))
        elif t == "ACTPOOL":
            if h % 2 or w % 2:
                continue
            L += [("PRELU",), ("SPATIAL_DROPOUT", 0, 0, 0, 0, 0.2), ("AVGPOOL2",)]; h //= 2; w //= 2
        elif t == "ACTMAXPOOL":
            if h % 2 or w % 2 or c % 4:
                continue
            L += [("PRELU",), ("MAXPOOL2",)] + ([("DROPOUT", 0, 0, 0, 0, 0.5)] if r.random() < 0.5 else []); h //= 2; w //= 2
        elif t in ("AVGPOOL2", "MAXPOOL2"):
            if h % 2 or w % 2 or (t == "MAXPOOL2" and c % 4):
                continue
            L.append((t,)); h //= 2; w //= 2
        elif t == "UPSAMPLE2X":
            if h * w > 64:
                continue
            L.append((t,)); h *= 2; w *= 2
        elif t == "SPATIAL_DROPOUT":
            L.append((t, 0, 0, 0, 0, 0.2))
        elif t == "DROPOUT":
            L.append((t, 0, 0, 0, 0, 0.5))
        elif t == "LEAKYRELU":
            L.append((t, 0, 0, 0, 0, 0.2))
        else:
            L.append((t,))
    return L, c, h, w


def _linear_tail(r, f, n, allow_one=True):
    """n draws behind a flatten; -> (layers, features)"""
    L = []
    pick = lambda xs: xs[int(r.integers(len(xs)))]
    for _ in range(n):
        t = pick(["LINEAR", "LINEAR", "LINEAR", "PRELU", "PRELUDROP", "DROPOUT", "SIGMOID", "LEAKYRELU"])
        if t == "LINEAR":
            o = pick(LINEAR_OUT if allow_one else LINEAR_OUT[1:])
            L.append(("LINEAR", f, o)); f = o
            if o == 1 and r.random() < 0.5:
                L.append(("SIGMOID",))
        elif t == "PRELUDROP":
            L += [("PRELU",), ("DROPOUT", 0, 0, 0, 0, 0.5)]
        elif t == "DROPOUT":
            L.append((t, 0, 0, 0, 0, 0.5))
        elif t == "LEAKYRELU":
            L.append((t, 0, 0, 0, 0, 0.2))
        else:
            L.append((t,))
    return L, f


def random_layer_lists(seed, n):
    """-> [(dims, layers, batch)]: n layer lists that are valid in Torch7, from every FG_* layer type.  No BatchNorm / SpatialDropout
    behind a flatten, MaxPool and BatchNorm only at C % 4 == 0, pools and stride 2 only on even maps (the header rules the rest out
    by construction).  What remains for fg_net_create to refuse: Linear(-> 1) behind a spatial flatten."""
    r = np.random.default_rng(seed)
    pick = lambda xs: xs[int(r.integers(len(xs)))]
    out = []
    while len(out) < n:
        B = int(pick([1, 2, 3, 4, 5, 8]))
        u = r.random()
        if u < 0.1:                                     # nn.ConcatTable: 2-4 branches that end in Linear, a tail
            c, h, w = pick(IN_C[:6]), int(r.integers(2, 9)), int(r.integers(2, 9))
            nb = int(r.integers(2, 5))
            L, tot = [("CONCAT_TABLE", nb)], 0
            for _ in range(nb):
                L.append(("BRANCH",))
                S, cc, hh, ww = _spatial_run(r, c, h, w, int(r.integers(0, 4)), in_branch=True)
                o = pick(LINEAR_OUT[1:])
                L += S + [("VIEW", cc * hh * ww), ("LINEAR", cc * hh * ww, o)] + ([("PRELU",)] if r.random() < 0.5 else [])
                tot += o
            T, f = _linear_tail(r, tot, int(r.integers(1, 4)))
            dims, L = (c, h, w), L + [("JOIN_TABLE",)] + T
        elif u < 0.25:                                  # a vector input with a Linear + View(C, H, W) head (G's first layers)
            f0, c, h, w = pick([8, 20, 100]), pick([4, 8, 12, 16]), int(r.integers(1, 5)), int(r.integers(1, 5))
            S, _, _, _ = _spatial_run(r, c, h, w, int(r.integers(0, 6)))
            dims, L = (f0, 1, 1), [("LINEAR", f0, c * h * w), ("VIEW", c, h, w)] + S
        else:
            c, h, w = pick(IN_C), int(r.integers(2, 17)), int(r.integers(2, 17))
            L, cc, hh, ww = _spatial_run(r, c, h, w, int(r.integers(1, 8)))
            if r.random() < 0.6:
                T, f = _linear_tail(r, cc * hh * ww, int(r.integers(1, 4)))
                L += [("VIEW", cc * hh * ww)] + T
                if T and T[-1][0] == "LINEAR" and T[-1][2] % 4 == 0 and T[-1][2] > 4 and r.random() < 0.5:       # ... and back to a map
                    o = T[-1][2]
                    L.append(("VIEW", o // 4, 2, 2))
                    L += _spatial_run(r, o // 4, 2, 2, int(r.integers(0, 3)))[0]
            dims = (c, h, w)
        if not L or not (len([l for l in L if l[0] not in MARKERS]) <= 11 or L[0][0] == "CONCAT_TABLE"):
            continue
        first, outs = walk(L, dims)                     # (raises if the grammar ever emits an invalid list)
        if max([int(np.prod(o.shape)) for o in outs] + [int(np.prod(first.shape))]) * B > 1 << 19:
            continue
        if any(l[0] == "LINEAR" and l[1] * l[2] > 1 << 21 for l in L):     # (parameters: a planning-only net allocates them too)
            continue
        out.append((tuple(int(v) for v in dims), [tuple(int(v) if not isinstance(v, (str, float)) else v for v in l) for l in L], B))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the two builders
# ---------------------------------------------------------------------------------------------------------------------------------
def _module(l, rng):
    from oracle import torch7_nn as O
    t, a, b, c, d, p, q = pad(l)
    if t == "LINEAR":
        return O.Linear(a, b, rng)
    if t == "VIEW":
        return O.View(a, b, c) if b > 0 else O.View(a)
    if t == "PRELU":
        return O.PReLU()
    if t == "UPSAMPLE2X":
        return O.SpatialUpSamplingNearest(2)
    if t == "CONV":
        s = 2 if p == 2 else 1
        if q > 1:
            return O.SpatialConvolutionUpsample(a, b // int(q * q), c, c, int(q), rng=rng)
        return O.SpatialConvolution(a, b, c, c, s, s, d, None, rng)
    if t == "BATCHNORM":
        return O.SpatialBatchNormalization(a, p if p > 0 else 1e-5, q if q > 0 else 0.1, rng)
    if t == "SPATIAL_DROPOUT":
        return O.SpatialDropout(p)
    if t == "AVGPOOL2":
        return O.SpatialAveragePooling()
    if t == "DROPOUT":
        return O.Dropout(p)
    if t == "SIGMOID":
        return O.Sigmoid()
    if t == "LEAKYRELU":
        return O.LeakyReLU(p)
    if t == "MAXPOOL2":
        return O.SpatialMaxPooling()
    raise ValueError(t)


def oracle_net(layers, dims, rng):
    """-> (net, mods): the oracle.torch7_nn module tree of the list (nn.Sequential; a table net is Sequential{ConcatTable{Sequential
    ...}, JoinTable, tail ...}) and its modules in the order of the list, None at the markers.  Parameters are non-trivial: the
    modules' own reset() (no zero bias in a convolution or a Linear), BatchNorm gamma in 0.5..1.5 and beta in -0.5..0.5, running
    statistics off their initial values, PReLU slopes in 0.1..0.4."""
    from oracle import torch7_nn as O
    net, cur, ct, mods = O.Sequential(), None, None, []
    cur = net
    for l in layers:
        if l[0] == "CONCAT_TABLE":
            ct = O.ConcatTable(); net.add(ct); mods.append(None)
        elif l[0] == "BRANCH":
            cur = O.Sequential(); ct.add(cur); mods.append(None)
        elif l[0] == "JOIN_TABLE":
            net.add(O.JoinTable()); cur = net; mods.append(None)
        else:
            m = _module(l, rng)
            if isinstance(m, O.PReLU):
                m.weight[0] = np.float32(rng.uniform(0.1, 0.4))
            if isinstance(m, O.SpatialBatchNormalization):
                m.weight[...] = rng.uniform(0.5, 1.5, m.nf); m.bias[...] = rng.uniform(-0.5, 0.5, m.nf)
                m.running_mean[...] = rng.uniform(-0.3, 0.3, m.nf); m.running_var[...] = rng.uniform(0.5, 2.0, m.nf)
            cur.add(m); mods.append(m)
    return net, mods


def sequentials(net):
    from oracle import torch7_nn as O
    return [net] + [b for m in net.modules if isinstance(m, O.ConcatTable) for b in m.modules]


def device_net(ctx, layers, dims, B):
    from face_generator_amd.runtime import DeviceNet
    return DeviceNet(ctx, [pad(l) for l in layers], tuple(dims), B)


def draw_masks(layers, dims, B, rng):
    """-> [oracle-shaped 0/1 mask per dropout layer], module order.  SpatialDropout: [B][C]; Dropout: the shape of its input."""
    first, outs = walk(layers, dims)
    masks = []
    for i, l in enumerate(layers):
        if l[0] == "SPATIAL_DROPOUT":
            masks.append((rng.random((B, outs[i].chw[0])) < 1 - pad(l)[5]).astype(np.float32))
        elif l[0] == "DROPOUT":
            masks.append((rng.random((B,) + outs[i].shape) < 1 - pad(l)[5]).astype(np.float32))
    return masks


def device_masks(layers, dims, masks):
    """the same masks in the order include/facegen_hip.h fixes: SpatialDropout [B][C], Dropout [B][features in internal NHWC order].
    The one place where NCHW becomes NHWC."""
    first, outs = walk(layers, dims)
    it, res = iter(masks), []
    for i, l in enumerate(layers):
        if l[0] == "SPATIAL_DROPOUT":
            res.append(next(it).reshape(-1))
        elif l[0] == "DROPOUT":
            res.append(to_device(next(it), outs[i]).reshape(-1))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# the device's PReLU / max-pool decisions -> the oracle (oracle/device_branches.py for any layer list: tables, a BatchNorm or a fused
# stage as the first one, pre-activations behind a flatten)
# ---------------------------------------------------------------------------------------------------------------------------------
def adopt(ctx, dn, layers, dims, mods, x, P, clear=False, also=()):
    """PReLU.pos_override / SpatialMaxPooling.indices_override of `mods` (and of the same positions of the lists in `also`) from the
    device's last forward.  The pre-activation is the stage output in front of the layer where fg_net_layer_output exposes it, the
    net's input x (NCHW numpy) for a first layer, z = bn_z(...) re-evaluated in float32 behind a BatchNorm, prelu(x) re-evaluated in
    float32 inside the fused PReLU + MaxPool stage.  Where the device exposes nothing the oracle keeps its own decision."""
    from oracle import torch7_nn as O
    first, outs = walk(layers, dims)
    B = x.shape[0]

    def dev_out(j):
        """the oracle-shaped float32 output of layer j as the device computed it; the net's input in front of a first layer"""
        if j < 0 or layers[j][0] == "BRANCH":
            return x.astype(np.float32)
        if layers[j][0] in MARKERS:
            return None
        t = exposed(dn, j)
        if t is None:
            return None
        return from_device(t.cpu().numpy().reshape(B, -1), outs[j]).astype(np.float32)

    for i, m in enumerate(mods):
        group = [m] + [o[i] for o in also]
        if isinstance(m, O.PReLU):
            pos = None
            if not clear and i > 0 and layers[i - 1][0] != "BRANCH":
                if isinstance(mods[i - 1], O.SpatialBatchNormalization):
                    xb = dev_out(i - 2)
                    mo, io, cc = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
                    ctx.check(ctx.lib.fg_net_bn_saved_stats(dn.h, i - 1, ctypes.byref(mo), ctypes.byref(io), ctypes.byref(cc)))
                    C = cc.value
                    mu = dn.ws[mo.value:mo.value + C].cpu().numpy().reshape(1, C, 1, 1)
                    istd = dn.ws[io.value:io.value + C].cpu().numpy().reshape(1, C, 1, 1)
                    wo, wn, bo, bn = dn.param_offsets(i - 1)
                    gam, bet = P[wo:wo + wn].reshape(1, C, 1, 1), P[bo:bo + bn].reshape(1, C, 1, 1)
                    if xb is not None:
                        z = (((xb - mu).astype(np.float32) * istd).astype(np.float32) * gam).astype(np.float32) + bet
                        pos = z.astype(np.float32) > 0
                else:
                    z = dev_out(i - 1)
                    pos = None if z is None else z > 0
            for g in group:
                g.pos_override = pos
        elif isinstance(m, O.SpatialMaxPooling):
            idx = None
            if not clear:
                xin = dev_out(i - 1) if (i == 0 or layers[i - 1][0] == "BRANCH" or ends_stage(dn, i - 1)) else None
                if xin is None and i > 0 and isinstance(mods[i - 1], O.PReLU):
                    xpre = dev_out(i - 2)
                    if xpre is not None:
                        a = np.float32(P[dn.param_offsets(i - 1)[0]])
                        xin = np.where(xpre > 0, xpre, (a * xpre).astype(np.float32)).astype(np.float32)
                if xin is not None:
                    n, c, h, w = xin.shape
                    idx = xin.reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4).argmax(axis=-1)
            for g in group:
                g.indices_override = idx


def exposed(dn, j):
    """the output of layer j where it ends a stage, None where the plan says it is fused inside one -- and nothing else: any other
    answer of fg_net_layer_output is an error"""
    from face_generator_amd._lib import FgError
    try:
        return dn.layer_output(j)
    except FgError as e:
        if "is fused inside a stage" not in str(e):
            raise
        return None


def ends_stage(dn, j):
    return exposed(dn, j) is not None


def flips(net):
    """-> (adopted PReLU decisions that differ from the oracle's own, PReLU units) after a forward with adopted branches"""
    from oracle import torch7_nn as O
    f = u = 0
    for s in sequentials(net):
        for m, xi in zip(s.modules, s._inputs):
            if isinstance(m, O.PReLU):
                u += int(xi.size)
                if m.pos_override is not None:
                    f += int(((xi > 0) != m.pos_override.reshape(xi.shape)).sum())
    return f, u


# ---------------------------------------------------------------------------------------------------------------------------------
# a case's operands and its references
# ---------------------------------------------------------------------------------------------------------------------------------
def operands(case, dtype=np.float64):
    """-> (net, mods, flat parameters, flat gradients, x, gy, masks): the oracle of the case in `dtype` with seeded parameters (the
    float32 values are what the device gets, whatever `dtype`), float32 inputs in -1..1, a normal output gradient, 0/1 masks"""
    from oracle import torch7_nn as O
    rng = np.random.default_rng(zlib.crc32(case.name.encode()) + case.seed)
    net, mods = oracle_net(case.layers, case.dims, rng)
    if case.gain != 1.0:
        for m in mods:
            if isinstance(m, O.SpatialConvolution):
                m.weight *= np.float32(case.gain)
    first, outs = walk(case.layers, case.dims)
    x = rng.uniform(-1, 1, (case.batch,) + first.shape).astype(np.float32)
    gy = rng.standard_normal((case.batch,) + outs[-1].shape).astype(np.float32)
    masks = draw_masks(case.layers, case.dims, case.batch, rng)
    net.astype(dtype)
    P, G = net.getParameters()
    return net, mods, P, G, x, gy, masks


def oracle_pass(net, G, x, gy, masks):
    """train forward + backward of the oracle in its own dtype -> (y, input gradient); module outputs stay in mods[i].output"""
    from oracle import torch7_nn as O
    O.set_dropout_masks(net, masks)
    net.training()
    dt = net.dtype
    y = net.forward(x.astype(dt))
    G[...] = 0
    return y, net.backward(x.astype(dt), gy.astype(dt))


def tensor_errors(net, got):
    """[(module, parameter name, offset, max |got - gradient of the module|)] over the flat vector `got`"""
    rows, off = [], 0
    for (m, pn, gn) in net.parameters():
        r = getattr(m, gn).reshape(-1)
        rows.append((m, pn, off, float(np.abs(got[off:off + r.size] - r).max())))
        off += r.size
    return rows


def reference_errors(case):
    """(e): the float32 oracle against the float64 oracle of the same net, inputs and masks, the float64 one on the float32 one's
    PReLU / max-pool decisions.  -> dict(flips, units, outputs, input_gradient, tensors={offset: error})"""
    from oracle import torch7_nn as O
    n32, m32, P32, G32, x, gy, masks = operands(case, np.float32)
    n64, m64, P64, G64, _, _, _ = operands(case, np.float64)
    assert np.array_equal(P32.astype(np.float64), P64)
    y32, gin32 = oracle_pass(n32, G32, x, gy, masks)
    for a, b, (s32, s64) in [(a, b, ss) for ss in zip(sequentials(n32), sequentials(n64)) for a, b in zip(ss[0].modules, ss[1].modules)]:
        if isinstance(a, O.PReLU):
            b.pos_override = s32._inputs[s32.modules.index(a)] > 0
        elif isinstance(a, O.SpatialMaxPooling):
            b.indices_override = a.indices
    y64, gin64 = oracle_pass(n64, G64, x, gy, masks)
    f, u = flips(n64)
    return dict(flips=f, units=u, outputs=float(np.abs(y32 - y64).max()), input_gradient=float(np.abs(gin32 - gin64).max()),
                tensors={off: e for (_, _, off, e) in tensor_errors(n64, G32.astype(np.float64))})


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name row dims layers batch math fusion expect absent guarded seed gain")
Case.__new__.__defaults__ = (0, 503, {}, {}, False, 0, 1.0)


def _sd(p=0.2):
    return ("SPATIAL_DROPOUT", 0, 0, 0, 0, p)


def _do(p=0.5):
    return ("DROPOUT", 0, 0, 0, 0, p)


def _conv(a, b, k=3, s=0, f=0):
    return ("CONV", a, b, k, (k - 1) // 2, s, f)


PR, BN, SIG, UP, AVG, MAXP = ("PRELU",), (lambda c: ("BATCHNORM", c)), ("SIGMOID",), ("UPSAMPLE2X",), ("AVGPOOL2",), ("MAXPOOL2",)
LK = ("LEAKYRELU", 0, 0, 0, 0, 0.2)

# `expect` / `absent`: {pass: [kernel name, ...]} that the case must / must not launch in that pass (fwd, eval, bwd3, bwd1, bwd2);
# tests/test_net_fusions_host.py (c) holds them to the planning-only log.  NET_CASES is filled below from these rows; the refused
# lists are REFUSED_CASES.
NET_CASES = []
REFUSED_CASES = []       # (name, row, dims, layers, part of the message)


def _case(name, row, dims, layers, batch, math=0, fusion=503, expect=None, absent=None, guarded=False, seed=0, gain=1.0):
    NET_CASES.append(Case(name, row, tuple(dims), [tuple(l) for l in layers], batch, math, fusion, expect or {}, absent or {}, guarded, seed, gain))


# ---- row 1: Linear + View(C, H, W) is one stage with a permuted output and a packed bias ---------------------------------------------
_G1 = [("LINEAR", 8, 48), ("VIEW", 12, 2, 2), BN(12), PR]
_case("r1-perm-bias-b8", 1, (8, 1, 1), _G1, 8, expect=dict(bwd3=["colsum_perm_kernel"]))
_case("r1-perm-bias-b1024-bn", 1, (8, 1, 1), _G1, 1024, expect=dict(bwd3=["colsum_perm_kernel"]), absent=dict(bwd3=["nhwc_to_nchw_kernel"]))
_case("r1-perm-bias-b1030", 1, (8, 1, 1), _G1, 1030, expect=dict(bwd3=["nhwc_to_nchw_kernel"]), absent=dict(bwd3=["colsum_perm_kernel"]), guarded=True)
# ---- row 2: flatten View + Linear with a pending NCHW permutation ----------------------------------------------------------------------
_case("r2-flatten-direct", 2, (3, 5, 4), [("VIEW", 60), ("LINEAR", 60, 10)], 3)
_case("r2-flatten-prelu", 2, (4, 3, 5), [("VIEW", 60), PR, ("LINEAR", 60, 7)], 3)
_case("r2-flatten-dropout", 2, (2, 4, 3), [_conv(2, 6), ("VIEW", 72), _do(), ("LINEAR", 72, 16)], 4)
_case("r2-flatten-leakyrelu", 2, (5, 2, 3), [("VIEW", 30), LK, ("LINEAR", 30, 5), PR], 2)
REFUSED_CASES.append(("r2-flatten-gemv-refused", 2, (3, 5, 4), [("VIEW", 60), ("LINEAR", 60, 1)], "Linear(->1) after a spatial flatten"))
REFUSED_CASES.append(("r2-flatten-prelu-gemv-refused", 2, (3, 5, 4), [("VIEW", 60), PR, ("LINEAR", 60, 1), SIG], "Linear(->1) after a spatial flatten"))
# ---- row 3: Linear(-> 1) [+ Sigmoid] is a GEMV stage --------------------------------------------------------------------------------------
_case("r3-gemv-sigmoid-last", 3, (100, 1, 1), [("LINEAR", 100, 70), PR, ("LINEAR", 70, 1), SIG], 5,
      expect=dict(fwd=["gemv_fwd_kernel"], bwd3=["gemv_bwd_act_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel", "sigmoid_bwd_kernel"]))
_case("r3-gemv-plain-inner", 3, (20, 1, 1), [("LINEAR", 20, 130), ("LINEAR", 130, 1), PR, ("LINEAR", 1, 4)], 3, expect=dict(fwd=["gemv_fwd_kernel"]))
_case("r3-gemv-dropout-mask", 3, (20, 1, 1), [("LINEAR", 20, 64), ("LINEAR", 64, 33), PR, _do(), ("LINEAR", 33, 1)], 6, expect=dict(bwd3=["gemv_bwd_act_kernel"]))
# ---- row 4: UPSAMPLE2X + CONV folded, and every reason not to fold ---------------------------------------------------------------------
_case("r4-fold-5x5", 4, (8, 4, 4), [UP, _conv(8, 16, 5)], 2, absent=dict(fwd=["upsample_fwd_kernel"]))
_case("r4-fold-3x3-odd-map", 4, (12, 3, 5), [UP, _conv(12, 8, 3), PR], 3, absent=dict(fwd=["upsample_fwd_kernel"]))
for _n, _c, _l in (("cin4", 4, _conv(4, 16, 3)), ("cout3", 8, _conv(8, 3, 3)), ("cin6", 6, _conv(6, 8, 3)), ("stride2", 8, _conv(8, 8, 3, 2)),
                   ("factor2", 8, _conv(8, 32, 3, 0, 2)), ("k7", 8, _conv(8, 8, 7))):
    _case("r4-nofold-" + _n, 4, (_c, 4, 4), [UP, _l], 2, expect=dict(fwd=["upsample_fwd_kernel"], bwd3=["upsample_bwd_kernel"]))
# ---- row 5: the conv classes as first, inner and last stage -------------------------------------------------------------------------------
_case("r5-thinin-general-thinoutsig", 5, (3, 6, 6), [_conv(3, 64), PR, _conv(64, 64), PR, _conv(64, 3), SIG], 2)
_case("r5-general-thinout-thinin", 5, (8, 8, 6), [_conv(8, 64, 5), _conv(64, 3), PR, _conv(3, 128, 5)], 2)
_case("r5-stride2-factor-stride2", 5, (16, 8, 8), [_conv(16, 32, 3, 2), _conv(32, 16, 3, 0, 2), _conv(4, 8, 3, 2)], 3,
      expect=dict(fwd=["nchw_review_kernel"], bwd3=["nchw_review_kernel", "zero_insert2_kernel"]))
_case("r5-factor-thinin-stride2-factor", 5, (4, 3, 4), [_conv(4, 12, 3, 0, 2), _conv(3, 64), _conv(64, 64, 3, 2), _conv(64, 8, 5, 0, 2)], 2,
      expect=dict(fwd=["nchw_review_kernel"]))
_case("r5-general-last-odd-map", 5, (8, 5, 7), [_conv(8, 8), LK, _conv(8, 12, 7)], 2)
_case("r5-thinout-first-1ch", 5, (64, 4, 6), [_conv(64, 1, 5), SIG, _conv(1, 64, 7), PR], 3)
_case("r5-thinout-factor2-sigmoid", 5, (64, 4, 4), [_conv(64, 4, 3, 0, 2), SIG], 2, expect=dict(fwd=["nchw_review_kernel", "sigmoid_fwd_kernel"]))
# ---- row 6: BATCHNORM [+ PRELU], batch statistics from the conv's epilogue ------------------------------------------------------------
_B6 = [_conv(8, 16), BN(16), PR]
_case("r6-bn-behind-winograd", 6, (8, 4, 4), _B6, 2, expect=dict(fwd=["wino_kernel"]), absent=dict(fwd=["bn_stats4_partial_kernel", "bn_stats_partial_kernel"]))
# (an implicit GEMM is un-split from M / 64 x Npad / 64 >= 384 tiles on: the smallest map with statistics in its epilogue)
_case("r6-bn-behind-igemm", 6, (8, 16, 16), _B6, 96, fusion=23, expect=dict(fwd=["igemm_kernel"]),
      absent=dict(fwd=["wino_kernel", "sum_splits_kernel", "bn_stats4_partial_kernel", "bn_stats_partial_kernel"]))
_case("r6-bn-behind-igemm-splitk", 6, (8, 4, 4), _B6, 2, fusion=23, expect=dict(fwd=["igemm_kernel", "sum_splits_kernel", "bn_stats4_partial_kernel"]))
_case("r6-bn-behind-igemm-math6-splitk", 6, (8, 4, 4), _B6, 2, math=6, fusion=23, expect=dict(fwd=["igemm_kernel", "sum_splits_kernel", "bn_stats4_partial_kernel"]))
# (bf16x6 planes exist only under the wave-specialised tile: from 256 blocks of 256 rows on, both channel counts % 16 == 0)
_case("r6-bn-behind-bf16x6", 6, (16, 32, 32), [_conv(16, 16), BN(16)], 64, math=6, fusion=23, expect=dict(fwd=["igemm_ws6_kernel", "bn_stats4_partial_kernel"]))
_case("r6-bn-behind-splitk-linear", 6, (16, 16, 16), [("VIEW", 4096), ("LINEAR", 4096, 64), ("VIEW", 16, 2, 2), BN(16)], 4,
      expect=dict(fwd=["sum_splits_kernel", "bn_stats4_partial_kernel"]))
_case("r6-bn-behind-thinin", 6, (3, 4, 6), [_conv(3, 64), BN(64), PR], 2, expect=dict(fwd=["bn_stats4_partial_kernel"]))
_case("r6-bn-behind-stride2", 6, (8, 8, 4), [_conv(8, 12, 3, 2), BN(12)], 3)
_case("r6-bn-behind-avgpool", 6, (8, 4, 4), [AVG, BN(8), PR, _conv(8, 8)], 2, expect=dict(fwd=["bn_stats4_partial_kernel"]))
_case("r6-bn-first", 6, (12, 2, 2), [BN(12), PR, _conv(12, 8)], 2, expect=dict(fwd=["bn_stats_partial_kernel"]))
# ---- row 7: PRELU + SPATIAL_DROPOUT + AVGPOOL2 -> one stage --------------------------------------------------------------------------------
_case("r7-actpool-fused", 7, (8, 4, 4), [_conv(8, 8), PR, _sd(), AVG, _conv(8, 8)], 3, expect=dict(fwd=["actpool_fwd_kernel"], bwd3=["actpool_bwd_kernel"]),
      absent=dict(fwd=["prelu_fwd_kernel", "avgpool_fwd_kernel"]))
_case("r7-actpool-unfused-c6", 7, (6, 4, 4), [_conv(6, 6), PR, _sd(), AVG, _conv(6, 6)], 3,
      expect=dict(fwd=["scale_mask_nc_kernel", "avgpool_fwd_kernel"], bwd3=["avgpool_bwd_kernel", "scale_mask_nc_kernel"]), absent=dict(fwd=["actpool_fwd_kernel"]))
_case("r7-actpool-first", 7, (8, 4, 6), [PR, _sd(), AVG, _conv(8, 4)], 3, expect=dict(fwd=["actpool_fwd_kernel"], bwd3=["actpool_bwd_kernel"]))
_case("r7-actpool-splitk", 7, (64, 2, 2), [_conv(64, 8, 7), PR, _sd(), AVG, ("VIEW", 8), ("LINEAR", 8, 5)], 1, guarded=True,
      expect=dict(fwd=["actpool_fwd_kernel"]), absent=dict(fwd=["sum_splits_kernel"]))
_case("r7-actpool-splitk-both", 7, (64, 4, 4), [_conv(64, 8, 7), PR, _sd(), AVG, _conv(8, 64, 7)], 1,
      expect=dict(fwd=["actpool_fwd_kernel"], bwd3=["actpool_bwd_kernel"]))
_case("r7-actpool-behind-linear-view", 7, (100, 1, 1), [("LINEAR", 100, 128), ("VIEW", 8, 4, 4), PR, _sd(), AVG], 3, fusion=23,
      expect=dict(fwd=["sum_splits_kernel", "actpool_fwd_kernel"]))
# ---- row 8: PRELU + MAXPOOL2 [+ DROPOUT] -> one stage --------------------------------------------------------------------------------------
_case("r8-actmaxpool", 8, (4, 4, 6), [_conv(4, 8), PR, MAXP, _conv(8, 4)], 3, expect=dict(fwd=["actmaxpool_fwd_kernel"], bwd3=["maxpool_prelu_bwd_kernel"]),
      absent=dict(fwd=["prelu_fwd_kernel", "maxpool_fwd_kernel"]))
_case("r8-actmaxpool-dropout", 8, (4, 6, 4), [_conv(4, 12), PR, MAXP, _do(), ("VIEW", 72), ("LINEAR", 72, 9)], 3,
      expect=dict(fwd=["actmaxpool_fwd_kernel"], eval=["actmaxpool_fwd_kernel"], bwd3=["maxpool_prelu_bwd_kernel"]), absent=dict(fwd=["mul_mask_kernel"]))
_case("r8-prelu-layer0-not-fused", 8, (8, 4, 4), [PR, MAXP, _conv(8, 8)], 2, expect=dict(fwd=["prelu_fwd_kernel", "maxpool_fwd_kernel"], bwd3=["maxpool_bwd_kernel", "prelu_bwd_kernel"]),
      absent=dict(fwd=["actmaxpool_fwd_kernel"]))
# ---- row 9: PRELU [+ DROPOUT] forward riding on the producer ------------------------------------------------------------------------------
_P9 = [_conv(8, 16), PR, _conv(16, 8)]
_Q9 = [("LINEAR", 20, 12), ("VIEW", 4, 3, 1), PR, _conv(4, 8)]          # (a Linear over <= 96 features is never split)
_case("r9-act-on-igemm", 9, (20, 1, 1), _Q9, 5, expect=dict(fwd=["igemm_act_kernel"], eval=["igemm_act_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-on-igemm-conv", 9, (8, 16, 16), [_conv(8, 16), PR], 96, fusion=23, expect=dict(fwd=["igemm_act_kernel"]), absent=dict(fwd=["prelu_fwd_kernel", "sum_splits_kernel"]))
_case("r9-act-on-splitsum-conv", 9, (8, 5, 4), _P9, 2, expect=dict(fwd=["sum_splits_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-on-winograd", 9, (8, 4, 4), _P9, 2, expect=dict(fwd=["wino_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-unfused-502", 9, (20, 1, 1), _Q9, 5, fusion=502, expect=dict(fwd=["prelu_fwd_kernel"], bwd3=["prelu_bwd_kernel"]), absent=dict(fwd=["igemm_act_kernel"]))
_case("r9-act-math6-splitsum", 9, (8, 5, 4), _P9, 2, math=6, expect=dict(fwd=["sum_splits_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-dropout-unsplit", 9, (20, 1, 1), [("LINEAR", 20, 12), PR, _do(), ("LINEAR", 12, 5)], 5, expect=dict(fwd=["prelu_fwd_kernel"]), absent=dict(fwd=["igemm_act_kernel"]))
_L9 = [("VIEW", 4096), ("LINEAR", 4096, 64), PR, _do(), ("LINEAR", 64, 10)]
_case("r9-act-on-splitsum-mask", 9, (16, 16, 16), _L9, 4, expect=dict(fwd=["sum_splits_kernel"], eval=["sum_splits_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"], eval=["prelu_fwd_kernel"]))
_case("r9-act-on-splitsum", 9, (16, 16, 16), [("VIEW", 4096), ("LINEAR", 4096, 64), PR, ("LINEAR", 64, 10)], 4, expect=dict(fwd=["sum_splits_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-on-thinin", 9, (3, 6, 4), [_conv(3, 64), PR, _conv(64, 8)], 2, absent=dict(fwd=["prelu_fwd_kernel"]))
_case("r9-act-on-thinin-5x5-pad", 9, (1, 6, 6), [_conv(1, 64, 5), PR, _conv(64, 8)], 2)
# ---- row 10: PRELU [+ DROPOUT] backward folded into the consumer ---------------------------------------------------------------------------
_P10 = [_conv(8, 8), _conv(8, 16), PR, _conv(16, 8)]
_case("r10-actbwd-on-winograd", 10, (8, 4, 4), _P10, 2, expect=dict(bwd3=["wino_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-actbwd-on-igemm", 10, (8, 5, 4), _P10, 2, absent=dict(bwd3=["prelu_bwd_kernel"], bwd1=["prelu_bwd_kernel"], bwd2=["prelu_bwd_kernel"]))
_case("r10-actbwd-math6-splitsum-folded", 10, (8, 5, 4), _P10, 2, math=6, fusion=23, expect=dict(bwd3=["sum_splits_actbwd_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-act-bf16x6-unfolded", 10, (16, 32, 32), [_conv(16, 16), PR, _conv(16, 16)], 64, math=6, fusion=23,
      expect=dict(fwd=["igemm_ws6_kernel", "prelu_fwd_kernel"], bwd3=["igemm_ws6_kernel", "prelu_bwd_kernel"]), absent=dict(fwd=["igemm_act_kernel"]))
_case("r10-actbwd-502-unfolded", 10, (8, 5, 4), _P10, 2, fusion=502, expect=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-prelu-stage1-folded", 10, (8, 5, 4), [_conv(8, 16), PR, _conv(16, 8)], 2, absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-gemv-prelu-stage0-unfolded", 10, (70, 1, 1), [PR, ("LINEAR", 70, 1), SIG], 5, expect=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-prelu-stage0-unfolded", 10, (8, 5, 4), [PR, _conv(8, 8)], 2, expect=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-actbwd-on-splitsum", 10, (8, 2, 9), [LK, _conv(8, 8), PR, _conv(8, 24, 3, 0, 2)], 8, fusion=23, expect=dict(bwd3=["sum_splits_actbwd_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-actbwd-on-splitsum-mask", 10, (16, 2, 2), [_conv(16, 16), _conv(16, 16), PR, _do(), _conv(16, 64, 7)], 1, expect=dict(bwd3=["sum_splits_actbwd_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-actbwd-cin6-sumsplits", 10, (6, 2, 2), [_conv(6, 6), _conv(6, 6), PR, _conv(6, 64, 7)], 1, expect=dict(bwd3=["prelu_bwd_kernel"]), absent=dict(bwd3=["sum_splits_actbwd_kernel"]))
_case("r10-actbwd-on-thinout", 10, (8, 4, 6), [_conv(8, 8), _conv(8, 64), PR, _conv(64, 3), SIG], 2, absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("r10-actbwd-on-thinout-7x7", 10, (8, 5, 16), [_conv(8, 8), _conv(8, 64, 5), PR, _conv(64, 3, 7)], 5, expect=dict(fwd=["thin_out_rows_mfma_kernel", "thin_out_rows_gather_kernel"]))
_case("r10-maxpool-behind-noop-view", 10, (4, 4, 4), [_conv(4, 8), _conv(8, 8), PR, ("VIEW", 8, 4, 4), MAXP, _conv(8, 4)], 3,
      expect=dict(fwd=["maxpool_fwd_kernel"], bwd3=["maxpool_prelu_bwd_kernel"]), absent=dict(fwd=["actmaxpool_fwd_kernel"], bwd3=["prelu_bwd_kernel", "maxpool_bwd_kernel"]))
_case("r10-actbwd-on-thinout-5x5-pow2", 10, (8, 4, 8), [_conv(8, 8), _conv(8, 64), PR, _conv(64, 1, 5)], 3, expect=dict(bwd3=["thin_in_mfma_pad_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
# ---- row 11: FG_FUSE_THIN_BIAS, FG_FUSE_WFINISH_BATCH across more weight-gradient layers than FG_DEFER_WMAX (16) --------------------
_DEEP = [_conv(3, 64), PR, _conv(64, 8)] + [_conv(8, 8)] * 17 + [("VIEW", 8 * 4 * 6), ("LINEAR", 192, 6)]
for _n, _f in (("default", 503), ("no-thin-bias", 503 & ~16), ("no-wfinish-batch", 503 & ~4)):
    _case("r11-deep-" + _n, 11, (3, 4, 6), _DEEP, 2, fusion=_f, gain=1.7)      # (20 layers deep: weights at unit gain, or no gradient reaches the first ones)
# ---- row 12: CONCAT_TABLE -------------------------------------------------------------------------------------------------------------------
_case("r12-table-2-branches", 12, (3, 4, 6), [("CONCAT_TABLE", 2), ("BRANCH",), ("VIEW", 72), ("LINEAR", 72, 5), ("BRANCH",), _conv(3, 8), PR, ("VIEW", 192),
                                              ("LINEAR", 192, 12), PR, ("JOIN_TABLE",), ("LINEAR", 17, 1), SIG], 3, expect=dict(bwd3=["sum_parts_kernel", "rows_join_split_kernel"]))
_case("r12-table-4-branches-actmaxpool-head", 12, (4, 4, 4),
      [("CONCAT_TABLE", 4), ("BRANCH",), PR, MAXP, ("VIEW", 16), ("LINEAR", 16, 3), ("BRANCH",), ("VIEW", 64), ("LINEAR", 64, 7), PR, _do(),
       ("BRANCH",), _conv(4, 8, 3, 2), LK, ("VIEW", 32), ("LINEAR", 32, 16), ("BRANCH",), PR, MAXP, _do(), ("VIEW", 16), ("LINEAR", 16, 2),
       ("JOIN_TABLE",), PR, ("LINEAR", 28, 6)], 3, guarded=True,
      expect=dict(fwd=["actmaxpool_fwd_kernel"], bwd3=["maxpool_prelu_bwd_kernel", "sum_parts_kernel"]))
# ---- from the sweep (tests/dispatch_audit.py net_sweep): signatures that no case above and no operator-level list launches ----------
_case("s-actbwd-on-igemm-linear", 10, (1, 4, 8), [SIG, ("VIEW", 32), _do(), PR, ("LINEAR", 32, 64)], 2, fusion=23, expect=dict(bwd3=["igemm_act_kernel"]), absent=dict(bwd3=["prelu_bwd_kernel"]))
_case("s-act-on-thinin-1ch", 9, (1, 7, 14), [_conv(1, 64), PR], 4, expect=dict(fwd=["thin_in_mfma_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("s-act-on-thinin-4ch", 9, (4, 6, 10), [_conv(4, 128), PR, _conv(128, 4)], 3, expect=dict(fwd=["thin_in_mfma_lds_kernel"]), absent=dict(fwd=["prelu_fwd_kernel"]))
_case("s-thinout-5x5-3ch", 5, (64, 8, 6), [_conv(64, 3, 5), SIG, _conv(3, 128, 5), _conv(128, 1)], 4, expect=dict(fwd=["thin_out_rows_mfma_kernel", "thin_out_rows_gather_kernel"]))
_case("s-thinout-7x7-1ch", 5, (64, 15, 8), [SIG, _conv(64, 1, 7), _conv(1, 32)], 1, expect=dict(fwd=["thin_out_rows_mfma_kernel", "thin_out_rows_gather_kernel"]))
