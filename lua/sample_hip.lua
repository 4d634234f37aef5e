--[[ sample_hip.lua -- the main() of sample.lua:69-115 re-hosted on the sampler level of libfacegen_hip.so (fg_sample /
fg_image_grid through FG.Sampler of lua/facegen_hip.lua).  Same globals (OPT, MODEL_G, MODEL_D, NN_UTILS), same pictures under
the same names: per run 1024 images, `random256_`, `random1024_`, `best_`, `worst_`, `random_` `%04d_base.jpg`.

What changes: the noise, G's and D's forward passes (chunks of OPT.batchSize, evaluate mode), the two rankings and the grids stay
on the device -- one C call for sample.lua:80-85, one per grid, and one copy back per finished picture.  D scores every image once
(the reference scores all of them again for "worst"; in evaluate mode that recomputes the same numbers).  Equal scores are
ordered by index (table.sort leaves that open).  With OPT.neighbours a sixth picture follows (sample.lua:91-99,
`best_%04d_neighbours_base.jpg`): the 16 best samples, each above its nearest training image.  The samples never leave the device;
the training set streams through fg_nearest_update (FG.Nearest) in chunks, and the first of equally near images wins like the
strict `<` of sample.lua:142.  The commented-out c2f chain is not part of this file.

NOT EXECUTED IN THIS REPOSITORY'S ENVIRONMENT (no Lua / Torch7 in the image); face_generator_amd/sample.py is the executed mirror
and tests/test_gpu_sampler.py checks the entries it calls.  Use from sample.lua once FG is bound (lua/patches/sample.lua.patch):
    SAMPLE = require 'sample_hip';  SAMPLE.main() ]]
local FG = require 'facegen_hip'
local sample = {}
sample.N = 1024
sample.stems = {'random256', 'random1024', 'best', 'worst', 'random'}

-- {D, G, opt, epoch} files under OPT.save_base; G and D may come from two files
function sample.loadModels()
    local loaded = {}
    local function checkpoint(name)
        if not loaded[name] then loaded[name] = torch.load(paths.concat(OPT.save_base, name)) end
        return loaded[name]
    end
    return checkpoint(OPT.G_base).G, checkpoint(OPT.D_base).D
end

-- nets on the device ({Copy, net, Copy} of NN_UTILS.activateCuda, the plan in :get(2).fg), evaluate mode
function sample.prepare()
    if not MODEL_G or not MODEL_D then MODEL_G, MODEL_D = sample.loadModels() end
    MODEL_G = NN_UTILS.activateCuda(MODEL_G)
    MODEL_D = NN_UTILS.activateCuda(MODEL_D)
    MODEL_G:evaluate()
    MODEL_D:evaluate()
end

-- the sampler lives as long as the two nets do
local function sampler()
    if not sample.sampler then
        local dnG, dnD = MODEL_G:get(2).fg, MODEL_D:get(2).fg
        assert(dnG and dnD, 'sample_hip: MODEL_G / MODEL_D carry no device plan (NN_UTILS.activateCuda first)')
        sample.sampler = FG.Sampler(dnG, dnD, sample.N, OPT.batchSize)
        sample.sampler:setSeed(OPT.seed, 0)
    end
    return sample.sampler
end

-- a reloaded pair of nets needs a new sampler
function sample.reset()
    sample.sampler = nil
end

-- which images go into a `random*` picture: the first n entries of a random permutation, as 0-based device indices
function sample.selectRandomImagesFrom(nImages, n)
    local shuffle = torch.randperm(nImages)
    local idx = {}
    for i = 1, math.min(n, nImages) do idx[i] = shuffle[i] - 1 end
    return FG.indexTensor(idx)
end

-- one finished picture: order = 'best' | 'worst' | an index tensor | nil (all images in their own order)
function sample.toGrid(s, order, k, nrow)
    return s:grid(order, k, nrow, 0, true)
end

-- D's scores at both ends of a ranking, for the log: {first, last} of the k best / worst
function sample.scoreRange(s, which, k)
    local preds = s:predictions()
    local order = s:order(which, k)
    return preds[order[1] + 1], preds[order[#order] + 1]
end

local function save(stem, run, grid, tail)
    local filename = paths.concat(OPT.writeto, string.format('%s_%04d_%s.jpg', stem, run, tail or 'base'))
    image.save(filename, grid)
    return filename
end

-- sample.lua:91-99 + findClosestNeighboursOf + toNeighboursGrid: the k best samples and their nearest training images as one
-- picture of nrow = k (sample 1, its neighbour, sample 2, ... in toDisplayTensor's order: the samples above, the neighbours below)
sample.neighbours = 16
sample.chunkRows = 8192
function sample.neighboursGrid(s, k)
    local c, h, w = s.dims[1], s.dims[2], s.dims[3]
    local elems = c * h * w
    -- [k samples ; k neighbours] NHWC: the samples by k device copies in the host order of the ranking
    local both = FG.DeviceTensor(2 * k * elems)
    local images = s:ptr(FG.C.FG_SAMPLER_IMAGES)
    for i, idx in ipairs(s:order('best', k)) do
        FG.check(FG.C.fg_d2d(FG.ctx, both.ptr + (i - 1) * elems, images + idx * elems, elems * 4))
    end
    -- the training set is stored CHW: convert the k queries once and stream the set as it is
    local queries = FG.DeviceTensor(k * elems)
    FG.check(FG.C.fg_nhwc_to_nchw(FG.ctx, both.ptr, queries.ptr, k, c, h, w))
    -- the set goes to HBM once (FG.Dataset) and every run searches it there: no upload per run, the neighbours gathered by index
    sample.trainingSet = sample.trainingSet or FG.Dataset(DATASET.loadImages(0, 9999999).data)
    local set = sample.trainingSet
    local N = set:size()
    local search = FG.Nearest(queries, k, elems)
    for first = 0, N - 1, sample.chunkRows do
        local n = math.min(sample.chunkRows, N - first)
        search:update({ptr = set.images.ptr + first * elems}, n, first)
    end
    local neighbours = FG.DeviceTensor(k * elems)
    FG.gatherImages(set.images, N, c, h, w, 1, {ptr = search.index}, k, neighbours, 0)      -- the device's own best_index
    FG.check(FG.C.fg_d2d(FG.ctx, both.ptr + k * elems, neighbours.ptr, k * elems * 4))
    local order = {}
    for i = 1, k do order[2 * i - 1], order[2 * i] = i - 1, k + i - 1 end
    return s:grid(FG.indexTensor(order), 2 * k, k, 0, true, both)
end

function sample.main()
    sample.prepare()
    local s = sampler()
    local written = {}
    os.execute(string.format("mkdir -p %s", OPT.writeto))
    print("Sampling...")
    for run = 1, OPT.runs do
        s:sample(sample.N, nil)
        local grids = {
            sample.toGrid(s, sample.selectRandomImagesFrom(sample.N, 256), 256, 16),
            sample.toGrid(s, nil, sample.N, 32),
            sample.toGrid(s, 'best', 64, 8),
            sample.toGrid(s, 'worst', 64, 8),
            sample.toGrid(s, sample.selectRandomImagesFrom(sample.N, 64), 64, 8),
        }
        for i, stem in ipairs(sample.stems) do
            written[#written + 1] = save(stem, run, grids[i])
        end
        if OPT.neighbours then
            written[#written + 1] = save('best', run, sample.neighboursGrid(s, sample.neighbours), 'neighbours_base')
        end
        local b1, b2 = sample.scoreRange(s, 'best', 64)
        local w1, w2 = sample.scoreRange(s, 'worst', 64)
        print(string.format("<sample> run %d: best %.4f .. %.4f, worst %.4f .. %.4f", run, b1, b2, w1, w2))
        xlua.progress(run, OPT.runs)
    end
    print("Finished.")
    return written
end

return sample
