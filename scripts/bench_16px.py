"""One G+D training iteration at --scale 16: (3,16,16), B = 128, G16 + create_D16_d, Adam, default options.
usage: python scripts/bench_16px.py <tree root> <timed iterations> <warm-up iterations>   -> one JSON line with ms per iteration
The tree is an argument so that two check-outs can be measured alternately by one caller (profiles/r07_16px_branched.md).  The loop
body is adversarial.train's: noise drawn inside the step on the fused route, S.next_noise on the host-driven route."""
import sys, time, json
root = sys.argv[1]
sys.path.insert(0, root)
import torch
from face_generator_amd import models, adversarial
from face_generator_amd.runtime import get_context
from face_generator_amd.state import S
steps, warm = int(sys.argv[2]), int(sys.argv[3])
ctx = get_context(0)
B = 128
S.reset()
G = models.create_G((3, 16, 16), 100).cuda(ctx, max_batch=B)
D = models.create_D((3, 16, 16)).cuda(ctx, max_batch=B)
tr = adversarial.Trainer(ctx, G, D, dict(batchSize=B, noiseDim=100))
real = ctx.uniform((B // 2, 16, 16, 3), 0.0, 1.0, seed=9)

def it():
    nz = None if tr.gan is not None else S.next_noise(ctx, B // 2, 100)
    tr.step_D(real, nz)
    tr.step_G(B if tr.gan is not None else S.next_noise(ctx, B, 100))

for _ in range(warm):
    it()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    it()
tr.finish_pending()
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / steps
print(json.dumps(dict(tree=root, fused=tr.gan is not None, ms_per_iteration=round(ms, 4), steps=steps, warmup=warm)))
