"""fg_nearest_update on the device (include/facegen_hip.h): the nearest row of a set to each of q queries, against numpy's restatement
of the header -- the difference rounded to fp32, its squares summed in fp64, the first arg-min.  Indices are compared exactly (the
inputs are asserted to leave a relative gap of 1e-9 between best and second best, far above the fp64 order error elems * 2^-52),
best_d2 within elems * 2^-52, best_dist exactly sqrt of the device's own d2.  Then: the same result bit for bit however the set is
cut into calls, the tie rule, NaN rows, the index range, the memory contract (tests/mem_contract.py), nn_utils.findClosestNeighboursOf
and the sixth picture of sample.main."""
import functools
import os

import numpy as np
import pytest
import torch

from mem_contract import Arena, run_contract, PATTERN

pytestmark = pytest.mark.gpu

FG_ERR_WORKSPACE = -5
SHAPES = [(33, 1000, 3072), (17, 257, 768), (16, 65, 257), (2, 64, 3), (15, 63, 255), (1, 1000, 1), (16, 64, 256), (16, 1, 3075)]
GAP = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from face_generator_amd.runtime import get_context
    return get_context(0)


def ref_d2(Q, R):
    """[q][n] float64: d = R - Q in fp32, squares summed in double"""
    out = np.empty((Q.shape[0], R.shape[0]))
    for j in range(Q.shape[0]):
        d = (R - Q[j][None]).astype(np.float32)
        out[j] = (d.astype(np.float64) ** 2).sum(-1)
    return out


def first_argmin(d2):
    """per query (index, d2) of the first smallest non-NaN entry; (-1, inf) where there is none"""
    idx, best = [], []
    for row in d2:
        ok = ~np.isnan(row)
        if not ok.any():
            idx.append(-1); best.append(np.inf)
            continue
        m = row[ok].min()
        i = int(np.flatnonzero(ok & (row == m))[0])
        idx.append(i); best.append(m)
    return np.array(idx, np.int64), np.array(best)


@functools.lru_cache(maxsize=None)
def case(q, n, elems, seed=0):
    rng = np.random.default_rng(1000 * seed + q + n + elems)
    Q, R = rng.random((q, elems), dtype=np.float32), rng.random((n, elems), dtype=np.float32)
    d2 = ref_d2(Q, R)
    idx, best = first_argmin(d2)
    # a condition on the inputs, checked on the reference alone: best and second best are far enough apart for an exact index
    if n > 1:
        two = np.sort(d2, axis=1)[:, :2]
        gap = (two[:, 1] - two[:, 0]) / two[:, 1]
        assert gap.min() >= GAP, "(%d, %d, %d): relative gap %g between best and second best" % (q, n, elems, gap.min())
    for a in (Q, R, d2, idx, best):
        a.setflags(write=False)
    return Q, R, d2, idx, best


def search(ctx, Q, R, cuts=None, first_index=0, row_offset=0, query_offset=0):
    """fg_nearest_update over R fed as calls of the lengths in `cuts` (then the rest); -> (best_d2 f64, best_index i32, best_dist f32)
    as numpy.  row_offset / query_offset: floats by which the device copies are shifted off their 16-byte alignment."""
    lib = ctx.lib
    q, elems = Q.shape
    n = R.shape[0]
    dev = ctx.device

    def shifted(a, off):
        buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + a.size]
        v.copy_(torch.tensor(a).reshape(-1))
        return v

    Qd, Rd = shifted(Q, query_offset), shifted(R, row_offset)
    d2 = torch.full((q,), -7.0, dtype=torch.float64, device=dev)
    idx = torch.full((q,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((q,), -7.0, dtype=torch.float32, device=dev)
    at, first = 0, 1
    for c in list(cuts or []) + [n]:
        c = min(c, n - at)
        if c <= 0:
            break
        nb = lib.fg_nearest_workspace_bytes(q, c)
        scratch = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=dev)
        ctx.check(lib.fg_nearest_update(ctx.h, Qd.data_ptr(), q, Rd.data_ptr() + 4 * at * elems, c, elems, first_index + at, first,
                                        d2.data_ptr(), idx.data_ptr(), dist.data_ptr(), scratch.data_ptr(), nb))
        at, first = at + c, 0
    assert at == n
    ctx.sync()
    return d2.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy()


def check_against_reference(got, idx, best, elems, first_index=0, what=""):
    d2, gi, dist = got
    assert np.array_equal(gi.astype(np.int64), np.where(idx >= 0, idx + first_index, -1)), what
    rel = np.abs(d2 - best) / np.where(best > 0, best, 1.0)
    print("%s: largest relative d2 error %.3g (bar %.3g)" % (what, rel.max(), elems * 2.0 ** -52))
    assert rel.max() <= elems * 2.0 ** -52, what
    assert np.array_equal(dist, np.sqrt(d2).astype(np.float32)), what                 # exactly the root of the device's own d2
    want = np.sqrt(best).astype(np.float32)
    assert np.all(np.abs(dist.astype(np.float64) - want) <= 2.0 ** -23 * want), what


@pytest.mark.parametrize("q,n,elems", SHAPES)
def test_indices_and_distances_equal_the_reference(ctx, q, n, elems):
    Q, R, _, idx, best = case(q, n, elems)
    check_against_reference(search(ctx, Q, R), idx, best, elems, what="(%d, %d, %d)" % (q, n, elems))


@pytest.mark.parametrize("q,n,elems", [(16, 64, 256), (17, 257, 768), (16, 1, 3075), (2, 64, 3)])
@pytest.mark.parametrize("row_offset,query_offset", [(1, 0), (0, 1), (3, 2)])
def test_unaligned_bases_take_the_scalar_loads_and_change_nothing(ctx, q, n, elems, row_offset, query_offset):
    Q, R, _, idx, best = case(q, n, elems)
    got = search(ctx, Q, R, row_offset=row_offset, query_offset=query_offset)
    check_against_reference(got, idx, best, elems, what="(%d, %d, %d) offsets %d, %d" % (q, n, elems, row_offset, query_offset))
    aligned = search(ctx, Q, R)
    assert np.array_equal(got[0].view(np.int64), aligned[0].view(np.int64))          # the order of the sum does not depend on the loads


@pytest.mark.parametrize("q,n,elems", [(33, 1000, 3072), (16, 65, 257)])
def test_chunked_feeding_is_bit_identical(ctx, q, n, elems):
    Q, R, _, idx, best = case(q, n, elems)
    whole = search(ctx, Q, R)
    cut = search(ctx, Q, R, cuts=[1, 7, 64])
    assert np.array_equal(whole[0].view(np.int64), cut[0].view(np.int64))
    assert np.array_equal(whole[1], cut[1]) and np.array_equal(whole[2].view(np.int32), cut[2].view(np.int32))
    check_against_reference(cut, idx, best, elems, what="(%d, %d, %d) in calls of 1, 7, 64 and the rest" % (q, n, elems))


def planted(q, n, elems, where, seed=3):
    """random Q, R with R[i] = Q[0] + noise for every i in `where` (equal copies): the nearest rows of query 0"""
    rng = np.random.default_rng(seed)
    Q, R = rng.random((q, elems), dtype=np.float32), rng.random((n, elems), dtype=np.float32)
    near = (Q[0] + rng.random(elems, dtype=np.float32) * np.float32(1e-3)).astype(np.float32)
    for i in where:
        R[i] = near
    return Q, R


@pytest.mark.parametrize("cuts", [None, [20], [6, 30], [5, 1, 34, 1]])
def test_equal_rows_the_earliest_wins(ctx, cuts):
    Q, R = planted(16, 100, 257, (5, 40))
    d2 = ref_d2(Q, R)
    assert d2[0, 5] == d2[0, 40] == d2[0].min()
    idx, best = first_argmin(d2)
    assert idx[0] == 5
    got = search(ctx, Q, R, cuts=cuts)
    check_against_reference(got, idx, best, 257, what="rows 5 and 40 equal, cuts %s" % (cuts,))


@pytest.mark.parametrize("n,where,cuts", [(100, (0,), None), (100, (99,), None), (64, (63,), None), (65, (64,), None), (100, (16,), [16]),
                                          (100, (15,), [16]), (100, (0, 99), [10, 80]), (100, (3, 98), [50])])
def test_winner_at_the_edges_of_a_call(ctx, n, where, cuts):
    """first and last row of a call; a winner in the first chunk with an equal copy in the last: the first stays"""
    Q, R = planted(3, n, 768, where)
    idx, best = first_argmin(ref_d2(Q, R))
    assert idx[0] == where[0]
    check_against_reference(search(ctx, Q, R, cuts=cuts), idx, best, 768, what="winner at %s of %d, cuts %s" % (where, n, cuts))


def test_a_query_equal_to_a_row_is_at_distance_zero(ctx):
    Q, R, _, _, _ = case(16, 65, 257)
    R = R.copy()
    R[33] = Q[4]
    d2, idx, dist = search(ctx, Q, R)
    assert idx[4] == 33 and d2[4] == 0.0 and dist[4] == 0.0 and not np.signbit(d2[4])


@pytest.mark.parametrize("cuts", [None, [10, 10]])
def test_nan_rows_never_win(ctx, cuts):
    Q, R = planted(5, 70, 300, (12,))
    R[12, 299] = np.nan                          # the row that would win
    R[30, 0] = np.nan
    d2 = ref_d2(Q, R)
    assert np.isnan(d2[:, 12]).all() and np.isnan(d2[:, 30]).all()
    idx, best = first_argmin(d2)
    assert 12 not in idx and 30 not in idx
    check_against_reference(search(ctx, Q, R, cuts=cuts), idx, best, 300, what="NaN rows, cuts %s" % (cuts,))
    # every row holds a NaN: nothing is found
    R[:, 7] = np.nan
    d2, gi, dist = search(ctx, Q, R, cuts=cuts)
    assert np.array_equal(gi, np.full(5, -1)) and np.all(np.isposinf(d2)) and np.all(np.isposinf(dist))


def test_indices_up_to_the_last_31_bit_value(ctx):
    Q, R, _, idx, best = case(16, 65, 257)
    base = (1 << 31) - 1 - 65
    got = search(ctx, Q, R, cuts=[30], first_index=base)
    check_against_reference(got, idx, best, 257, first_index=base, what="first_index = 2^31 - 1 - n")
    assert got[1].min() >= base and got[1].max() <= (1 << 31) - 2


@pytest.mark.parametrize("q,n,elems,row_align", [(33, 1000, 3072, 256), (16, 65, 257, 256), (17, 257, 768, 4), (2, 64, 3, 256)])
def test_memory_contract(ctx, q, n, elems, row_align):
    """Guard bands around scratch and the three result buffers, scratch and results pre-filled with NaN, 0 and 1e30, NaN behind the
    inputs: nothing outside is written, the inputs stay, and the result does not depend on the fills.  Scratch is exactly
    fg_nearest_workspace_bytes long; one byte less is refused before anything is written."""
    lib = ctx.lib
    Q, R, _, idx, best = case(q, n, elems)
    nb = lib.fg_nearest_workspace_bytes(q, n)
    assert nb % 8 == 0
    ar = Arena.sized(ctx.device, [Q.size, R.size, 2 * q, q, q, nb // 4])
    Qd, Rd = ar.put(Q.copy(), name="queries"), ar.put(R.copy(), align=row_align, name="rows")
    d2, gi, dist = ar.take(2 * q, name="best_d2"), ar.take(q, name="best_index"), ar.take(q, name="best_dist")
    scratch = ar.take(nb // 4, name="scratch")
    P = lambda t: t.data_ptr()
    seen = []

    def call():
        ctx.check(lib.fg_nearest_update(ctx.h, P(Qd), q, P(Rd), n, elems, 0, 1, P(d2), P(gi), P(dist), P(scratch), nb))
        ctx.sync()
        seen.append((d2.view(torch.float64).cpu().numpy().copy(), gi.view(torch.int32).cpu().numpy().copy()))

    # best_d2 (doubles) and best_index (ints) are not fp32 data: they are pre-filled like workspaces and compared here
    (do,) = run_contract(ar, call, [Qd, Rd], [dist], [d2, gi, scratch], what="fg_nearest_update (%d, %d, %d)" % (q, n, elems))
    assert len(seen) == 3
    for other in seen[1:]:
        assert np.array_equal(seen[0][0].view(np.int64), other[0].view(np.int64)) and np.array_equal(seen[0][1], other[1])
    check_against_reference((seen[0][0], seen[0][1], do.cpu().numpy()), idx, best, elems, what="contract (%d, %d, %d)" % (q, n, elems))
    # one byte short: refused, nothing written
    for v in (d2, gi, dist, scratch):
        v.view(torch.int32).fill_(PATTERN)
    rc = lib.fg_nearest_update(ctx.h, P(Qd), q, P(Rd), n, elems, 0, 1, P(d2), P(gi), P(dist), P(scratch), nb - 1)
    ctx.sync()
    assert rc == FG_ERR_WORKSPACE and "scratch" in lib.fg_last_error(ctx.h).decode()
    ar.assert_guards("one byte short")
    for v in (d2, gi, dist, scratch):
        assert bool((v.view(torch.int32) == PATTERN).all())


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_find_closest_neighbours_of(ctx):
    from face_generator_amd import nn_utils
    rng = np.random.default_rng(77)
    train = rng.random((300, 3, 16, 16), dtype=np.float32)
    queries = rng.random((16, 3, 16, 16), dtype=np.float32)
    plant = {0: 299, 3: 0, 5: 128, 9: 17, 12: 64, 15: 255}
    for j, i in plant.items():
        queries[j] = train[i] + rng.random((3, 16, 16), dtype=np.float32) * np.float32(1e-3)
    d2 = ref_d2(queries.reshape(16, -1), train.reshape(300, -1))
    idx, best = first_argmin(d2)
    two = np.sort(d2, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) / two[:, 1]).min() >= GAP
    images = torch.from_numpy(np.ascontiguousarray(queries.transpose(0, 2, 3, 1))).to(ctx.device)        # device NHWC

    class Set:                                   # what dataset.lua returns: size() and [i]
        def size(self):
            return 300

        def __getitem__(self, i):
            return torch.from_numpy(train[i])

    for ts, chunk in ((torch.from_numpy(train), 8192), (train, 128), (Set(), 77)):
        found, neighbours = nn_utils.findClosestNeighboursOf(images, ts, chunk_rows=chunk, ctx=ctx)
        assert [i for i, _ in found] == idx.tolist()
        for j, i in plant.items():
            assert found[j][0] == i
        want = np.sqrt(best).astype(np.float32).astype(np.float64)
        assert np.all(np.abs(np.array([d for _, d in found]) - want) <= 2.0 ** -23 * want)
        assert neighbours.shape == (16, 3, 16, 16) and np.array_equal(neighbours.numpy(), train[idx])


def test_sample_main_writes_the_sixth_picture(ctx, tmp_path, monkeypatch):
    """A small G / D pair at 16 px and a .npy set: the sixth picture is fg_image_grid over [16 best ; their neighbours] in the order
    0, 16, 1, 17, ..; the five other files are byte-equal to a run without the flag at the same seed."""
    from test_gpu_sampler import oracle_nets, device_nets, ref_grid
    from face_generator_amd import sample
    from face_generator_amd.runtime import Sampler
    from face_generator_amd.state import S
    S.reset()
    st, _ = oracle_nets(2312, 16)
    G, D = device_nets(ctx, st, 16, 16)
    rng = np.random.default_rng(9)
    train = rng.random((300, 3, 16, 16), dtype=np.float32)
    np.save(str(tmp_path / "set.npy"), train)
    saved = {}
    real_save = sample.save_picture

    def keep(path, grid):
        saved[path] = grid.clone()
        real_save(path, grid)

    monkeypatch.setattr(sample, "loadModels", lambda opt, dims: (G, D))
    monkeypatch.setattr(sample, "save_picture", keep)
    base = dict(scale=16, gpu=0, batchSize=16, runs=1, seed=5)
    plain = sample.main(dict(base, writeto=str(tmp_path / "plain")), ctx)
    six = sample.main(dict(base, writeto=str(tmp_path / "six"), neighbours=True, trainingSet=str(tmp_path / "set.npy")), ctx)
    S.reset()
    assert len(plain) == 5 and len(six) == 6 and os.path.basename(six[5]).startswith("best_0001_neighbours_base.")
    for a, b in zip(plain, six):
        assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read(), a
    assert os.path.isfile(six[5]) and os.path.getsize(six[5]) > 0
    grid = saved[six[5]].numpy()
    assert grid.shape == (3, 2 * 16, 16 * 16)
    # the same samples again from a sampler of the test's own, the neighbours from the reference
    sm = Sampler(ctx, G._inner().device_net, D._inner().device_net, sample.N_IMAGES, 16)
    sm.set_seed(5, 0)
    sm.sample(sample.N_IMAGES)
    order = sm.view("ORDER_DESC")[:16].cpu().numpy()
    best16 = sm.view("IMAGES").cpu().numpy()[order]                                     # NHWC
    d2 = ref_d2(np.ascontiguousarray(best16.transpose(0, 3, 1, 2)).reshape(16, -1), train.reshape(300, -1))
    idx, _ = first_argmin(d2)
    two = np.sort(d2, axis=1)[:, :2]
    assert ((two[:, 1] - two[:, 0]) / two[:, 1]).min() >= GAP
    both = np.concatenate([best16, np.ascontiguousarray(train[idx].transpose(0, 2, 3, 1))])
    inter = np.arange(32).reshape(2, 16).T.reshape(-1)
    assert inter[:4].tolist() == [0, 16, 1, 17]
    dev_grid = sm.grid(torch.from_numpy(inter.astype(np.int32)).to(ctx.device), 32, 16, padding=0, normalize=True,
                       images=torch.from_numpy(both).to(ctx.device)).cpu().numpy()
    assert np.array_equal(grid, dev_grid)
    want, _ = ref_grid(both, inter, 32, 16, 0, True)
    assert np.abs(grid - want).max() <= 1e-6


def test_training_set_from_a_directory_of_pictures(ctx, tmp_path):
    """--trainingSet DIR: sorted files, 8-bit values / 255 in CHW; a picture of the sampled size passes image.scale unchanged, a
    larger one comes out at the sampled size within [0, 1]."""
    from face_generator_amd import sample
    rng = np.random.default_rng(4)
    small = rng.integers(0, 256, (2, 3, 16, 16), dtype=np.uint8)
    for i in range(2):
        sample.save_picture(str(tmp_path / "set" / ("b%d.ppm" % i)), torch.from_numpy(small[i].astype(np.float32) / 255.0))
    sample.save_picture(str(tmp_path / "set" / "a_large.ppm"), torch.rand(3, 40, 24))
    if sample.picture_extension() is None:               # no PIL: the directory form is refused by name, a .npy is asked for
        with pytest.raises(ValueError, match="PIL"):
            sample.loadTrainingSet(str(tmp_path / "set"), (3, 16, 16), ctx)
        return
    data = sample.loadTrainingSet(str(tmp_path / "set"), (3, 16, 16), ctx)
    assert tuple(data.shape) == (3, 3, 16, 16) and data.dtype == torch.float32
    assert np.array_equal(data[1:].numpy(), small.astype(np.float32) / np.float32(255.0))
    assert float(data[0].min()) >= 0.0 and float(data[0].max()) <= 1.0 and float(data[0].std()) > 0.01
