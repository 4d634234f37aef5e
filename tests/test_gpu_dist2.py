"""End-to-end data parallelism with TWO real processes (both on the single GPU of the test box, collectives over gloo --
RCCL refuses two ranks on one device): one D-step + one G-step of `adversarial.Trainer` with the batch sharded over the
ranks (deferred D all-reduce, bucketed backward-overlapped G all-reduce, 1/world in the fused Adam, sync-BN) must give the
parameters of a single process run on the global batch, and the replicas must agree bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist2_worker.py")


def test_two_process_sharded_step_equals_global_batch(tmp_path):
    from gpu_util import close_after_first_adam_step
    B = 16
    prefix = str(tmp_path / "dp")
    env = dict(os.environ)
    r = subprocess.run([sys.executable, WORKER, "0", "1", str(B), prefix], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), "2", str(B), prefix, "29577"], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env) for k in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    one = np.load(prefix + "_0_of_1.npz")
    r0, r1 = np.load(prefix + "_0_of_2.npz"), np.load(prefix + "_1_of_2.npz")
    for k in ("pG", "pD", "gG", "gD"):
        assert np.array_equal(r0[k], r1[k]), "replicas diverged in %s" % k
    # all-reduced SUM of the shard gradients (each a mean over B/2 rows) = 2 x the global-batch mean gradient
    # (G's gradient is taken through the D that was just updated by Adam -- whose step is sign-like, so near-zero D
    #  gradients may legitimately move a D parameter differently in the two runs -- hence the wider bar for G)
    for net, rel in (("D", 1e-4), ("G", 1e-3)):
        g_one, g_two = one["g" + net], 0.5 * r0["g" + net]
        assert np.abs(g_two - g_one).max() <= rel * np.abs(g_one).max() + 1e-7, net
        close_after_first_adam_step(r0["p" + net], one["p" + net], g_two, g_one, "%s parameters, 2 ranks vs global batch" % net)


def test_two_process_default_per_gpu_batchnorm_keeps_replicas_identical(tmp_path):
    """The default (throughput) mode: per-GPU BatchNorm statistics, deferred D all-reduce, bucketed G all-reduce."""
    prefix = str(tmp_path / "dp_local_bn")
    env = dict(os.environ)
    procs = [subprocess.Popen([sys.executable, WORKER, str(k), "2", "16", prefix, "29579", "0"], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, env=env) for k in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    r0, r1 = np.load(prefix + "_0_of_2.npz"), np.load(prefix + "_1_of_2.npz")
    for k in ("pG", "pD", "gG", "gD"):
        assert np.isfinite(r0[k]).all() and np.array_equal(r0[k], r1[k]), "replicas diverged in %s" % k


def test_bench_multi_rank_control_flow_on_one_gpu():
    """bench.py under torch.distributed.run with TWO ranks (test hook: both on device 0, gloo): barriers, MAX-over-ranks
    timing, the supplementary bf16x6 leg and the profiled iterations all contain collectives and must not dead-lock."""
    import json
    env = dict(os.environ, FG_BENCH_TEST_GLOO="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29583", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--batch", "16", "--full", "--c2f-steps", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 32 and j["value"] > 0 and j["scaling"] == "weak"
    assert "alt_math" in j and "error" not in j["alt_math"] and "roofline" in j and "cpu_baseline" not in j
    assert j["collective_fallback"] is False and j["rccl_ranks_seen"] == 2          # (gloo was ASKED for here: not a fallback)
    # round 4: the run diagnoses itself -- every rank's own step time (a straggler shows), and the collective schedule of all N
    # ranks walked on the CPU before the rendezvous (rank 0, planning-only contexts), with its hash in the line
    assert len(j["per_rank_ms_per_step"]) == 2 and all(0 < v <= j["ms_per_step"] * 1.001 + 0.05 for v in j["per_rank_ms_per_step"])
    d = j["dry_collective"]
    assert d["ranks_agree"] is True and d["ranks_walked"] == 2 and len(d["schedule_sha16"]) == 16 and d["this_run"], d
    assert any(" allreduce f32 2863239 " in l for l in d["this_run"])                  # D's flat gradient, models.lua:382-416
    # round 5: the legs a first SCALE record needs -- each rank's compute-only time and what it leaves of the
    # step (scaling efficiency from THIS run alone), the other BatchNorm mode, the strong-scaling split of the global batch of 128
    assert len(j["per_rank_compute_ms"]) == 2 and all(v > 0 for v in j["per_rank_compute_ms"])
    # two 3-step timed regions of two processes that SHARE one GPU: the ratio is a plausibility check of the field (it exists, it is
    # a positive ratio of the right order), not a measurement -- round 6 saw 1.25 on an otherwise green run
    assert 0 < j["compute_over_step"] <= 3.0, j["compute_over_step"]
    assert abs(j["exchange_exposed_ms_per_step"] - (j["ms_per_step"] - max(j["per_rank_compute_ms"]))) < 1e-9
    mg = j["multi_gpu"]
    assert set(mg) == {"compute_only", "sync_bn", "strong"}, sorted(mg)
    for name, leg in mg.items():
        assert "error" not in leg, (name, leg)
        assert leg["value"] > 0 and leg["ms_per_step"] > 0 and len(leg["per_rank_ms_per_step"]) == 2 and leg["note"], (name, leg)
    assert mg["compute_only"]["batch_per_gpu"] == 16 and mg["sync_bn"]["batch_per_gpu"] == 16 and mg["strong"]["batch_per_gpu"] == 64
    c = j["c2f"]                                                                     # configs[4]-style: B/2 per rank, D_it = 2
    assert "error" not in c, c
    assert c["value"] > 0 and c["config"]["batch_per_gpu"] == 8 and "D_it=2" in c["config"]["workload"]


def test_bench_watchdog_prints_a_partial_line_naming_the_stage():
    """A multi-GPU bench run that stops making progress (rendezvous, ncclCommInitRank, a collective one rank never joins) must not run
    silently into the driver's limit: past --watchdog rank 0 prints ONE partial JSON line (error, stage, whatever was measured) and
    every rank exits 4.  Forced here with a watchdog far shorter than the run."""
    import json
    env = dict(os.environ, FG_BENCH_TEST_GLOO="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29587", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--batch", "16", "--full", "--c2f-steps", "1", "--watchdog", "0.3", "--no-dry-check"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["partial"] is True and j["n_gpus"] == 2 and j["stage"] and "did not finish" in j["error"] and j["stage"] in j["error"]
    assert "metric" in j and "value" in j                      # whatever was measured by then (None before the timed steps)


def _two_gpus():
    import torch
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs (one rank per device: RCCL refuses two ranks on one)")
@pytest.mark.parametrize("sync_bn", ["1", "0"])
def test_library_bound_rccl_exchange_on_two_gpus_equals_torch_distributed(tmp_path, sync_bn):
    """The path the 8-GPU bench takes and the one-GPU box cannot run: fg_step_D / fg_step_G with the gradient exchange issued BY THE
    LIBRARY on its own communicator (fg_comm_*: RCCL bound through the C ABI, the exchange stream, the deferred D all-reduce, the
    bucketed G all-reduce behind the backward stages, sync-BN's fp64 sums).  Two ranks on two devices: (a) the replicas stay
    bit-identical, (b) the result equals bit for bit what torch.distributed (backend nccl = RCCL) gives as the carrier of the same
    closures -- a two-operand sum has one order -- and (c) with sync-BN it matches the single-process run on the global batch."""
    from gpu_util import close_after_first_adam_step
    B = 16
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = {}
    for carrier, port in (("fg_comm", "29583"), ("nccl", "29585")):
        prefix = str(tmp_path / ("dp_" + carrier))
        procs = [subprocess.Popen([sys.executable, WORKER, str(k), "2", str(B), prefix, port, sync_bn, carrier], stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, text=True, env=env) for k in range(2)]
        outs = [p.communicate(timeout=900) for p in procs]
        for p, (so, se) in zip(procs, outs):
            assert p.returncode == 0, se[-3000:]
        res[carrier] = (np.load(prefix + "_0_of_2.npz"), np.load(prefix + "_1_of_2.npz"))
        for k in ("pG", "pD", "gG", "gD"):
            assert np.isfinite(res[carrier][0][k]).all() and np.array_equal(res[carrier][0][k], res[carrier][1][k]), \
                "%s: replicas diverged in %s" % (carrier, k)
    for k in ("pG", "pD", "gG", "gD"):
        assert np.array_equal(res["fg_comm"][0][k], res["nccl"][0][k]), "fg_comm and torch.distributed(nccl) differ in %s" % k
    if sync_bn == "1":
        prefix = str(tmp_path / "one")
        r = subprocess.run([sys.executable, WORKER, "0", "1", str(B), prefix], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        one, r0 = np.load(prefix + "_0_of_1.npz"), res["fg_comm"][0]
        for net, rel in (("D", 1e-4), ("G", 1e-3)):
            g_one, g_two = one["g" + net], 0.5 * r0["g" + net]
            assert np.abs(g_two - g_one).max() <= rel * np.abs(g_one).max() + 1e-7, net
            close_after_first_adam_step(r0["p" + net], one["p" + net], g_two, g_one, "%s parameters, 2 GPUs vs global batch" % net)
