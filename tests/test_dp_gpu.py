"""Data-parallel equivalence on the GPU (SURVEY.md §4 tier 4): two ranks, each on its shard of the
global batch with the 1/world loss seed + SUM all-reduce of the flat gradient buffer, must reproduce
the single-process full-batch gradients and the same optimizer step.  The test box has one GPU, so
both ranks share device 0 and use the gloo backend (SRK_DIST_BACKEND / SRK_SINGLE_GPU test switches
of dp.init_from_env); the RCCL path differs only in the transport."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, out, backend="gloo"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SRK_DIST_BACKEND=backend)
    if backend == "gloo":
        os.environ["SRK_SINGLE_GPU"] = "1"   # both ranks share device 0
    sys.path.insert(0, ROOT)
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    r, w, local = pkg.dp.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    gb = 6
    x, t = fill.rand((gb, 3, 8, 8), 1), fill.rand((gb, 3, 32, 32), 2)

    def make():
        net = pkg.EDSRNet(3, 64, 4)
        fill.fill_module(net, 7, 0.5)
        net.to(dev).train()
        flat = pkg.optim.FlatParams(net)
        return net, flat, pkg.optim.make_optimizer("edsr", flat, 1e-3)

    # data-parallel step on this rank's shard
    net, flat, opt = make()
    dp = pkg.dp.DataParallel(flat, bucket_bytes=1 << 20)
    dp.broadcast_params()
    step = pkg.trainers.l1_step(net, opt, dp)
    lo, hi = pkg.dp.shard_range(gb, r, w)
    loss = step(x[lo:hi].to(dev), t[lo:hi].to(dev))
    g_dp, p_dp = flat.grad.clone().cpu(), flat.data.clone().cpu()
    # the same shard gradient exchanged as ONE all-reduce after all weight gradients (no overlap, no buckets): the
    # overlapped, bucketed exchange must give bit-identical sums
    net_s, flat_s, opt_s = make()
    opt_s.zero_grad()
    with pkg.ops.manual_wgrad_flush():
        pkg.ops.l1_loss(net_s(x[lo:hi].to(dev)), t[lo:hi].to(dev)).backward(dp.loss_seed)
    n_groups = len(pkg.ops.pending_wgrad_groups(dp.trunk_chunk_layers))
    sends = dp.__class__(flat_s, trunk_chunk_layers=dp.trunk_chunk_layers).plan(pkg.ops.pending_wgrad_groups(dp.trunk_chunk_layers))
    pkg.ops.flush_wgrads()
    torch.distributed.all_reduce(flat_s.grad)
    g_single = flat_s.grad.clone().cpu()
    # graph-captured DP step from the same start (second model)
    net2, flat2, opt2 = make()
    dp2 = pkg.dp.DataParallel(flat2)
    snap = flat2.data.clone()
    gstep = pkg.trainers.GraphedStep(net2, opt2, pkg.ops.l1_loss, (x[lo:hi].to(dev), t[lo:hi].to(dev)), dp=dp2,
                                     warmup=1)
    flat2.data.copy_(snap)
    opt2.exp_avg.zero_(); opt2.exp_avg_sq.zero_(); opt2.step_dev.zero_()
    gstep(x[lo:hi].to(dev), t[lo:hi].to(dev))
    p_graph = flat2.data.clone().cpu()
    # SRGAN: eager DP step vs the step as graphs split at the two exchanges (trainers.GraphedSegments)
    def make_gan():
        G, D = pkg.SRGANGenerator(3, 16, 2), pkg.SRGANDiscriminator(3, 8, 32)
        fill.fill_module(G, 5, 0.7)
        fill.fill_module(D, 6, 1.0)
        G.to(dev).train()
        D.to(dev).train()
        gf, df = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
        return G, D, pkg.optim.make_optimizer("srgan_g", gf, 1e-3), pkg.optim.make_optimizer("srgan_d", df, 1e-2), \
            pkg.dp.DataParallel(gf), pkg.dp.DataParallel(df)

    lr_img, hr_img = fill.rand((4, 3, 8, 8), 31)[2 * r:2 * r + 2].to(dev), fill.rand((4, 3, 32, 32), 32)[2 * r:2 * r + 2].to(dev)
    G, D, g_opt, d_opt, gan_gdp, gan_ddp = make_gan()
    sstep = pkg.trainers.srgan_step(G, D, g_opt, d_opt, gan_gdp, gan_ddp)
    gan_losses = [[float(v) for v in sstep(lr_img, hr_img)] for _ in range(2)]
    gan_p = torch.cat([g_opt.flat.data, d_opt.flat.data]).cpu()

    def state(o):
        return [o.flat.data] + [getattr(o, k) for k in ("buf", "exp_avg", "exp_avg_sq", "step_dev") if getattr(o, k, None) is not None]

    G2, D2, g_opt2, d_opt2, g_dp2, d_dp2 = make_gan()
    snap = [[t_.clone() for t_ in state(o)] for o in (g_opt2, d_opt2)]
    bn = [(m, m.running_mean.clone(), m.running_var.clone()) for net_ in (G2, D2) for m in net_.modules()
          if isinstance(m, torch.nn.BatchNorm2d)]
    seg = pkg.trainers.GraphedSegments(pkg.trainers.srgan_segments(G2, D2, g_opt2, d_opt2, g_dp2, d_dp2), (lr_img, hr_img),
                                       warmup=1)
    for o, saved in zip((g_opt2, d_opt2), snap):
        for t_, t0 in zip(state(o), saved):
            t_.copy_(t0)
    for m, rm, rv in bn:
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    gan_losses_graph = [[float(v) for v in seg(lr_img, hr_img)] for _ in range(2)]
    gan_p_graph = torch.cat([g_opt2.flat.data, d_opt2.flat.data]).cpu()
    # SyncBN (SURVEY.md 8e caveat): with the [2C] BatchNorm sums all-reduced, the data-parallel step normalises with the
    # statistics of the GLOBAL batch -- eager, and as graphs cut again at every statistics all-reduce (trainers._Splitter)
    def bn_state(*nets):
        return torch.cat([t_.flatten().float() for net_ in nets for m in net_.modules() if isinstance(m, torch.nn.BatchNorm2d)
                          for t_ in (m.running_mean, m.running_var)]).cpu()

    G3, D3, g_opt3, d_opt3, g_dp3, d_dp3 = make_gan()
    n_sync = pkg.trainers.sync_batchnorm(G3) + pkg.trainers.sync_batchnorm(D3)
    s3 = pkg.trainers.srgan_step(G3, D3, g_opt3, d_opt3, g_dp3, d_dp3)
    sync_losses = [float(v) for v in s3(lr_img, hr_img)]
    sync_p, sync_bn = torch.cat([g_opt3.flat.data, d_opt3.flat.data]).cpu(), bn_state(G3, D3)
    G4, D4, g_opt4, d_opt4, g_dp4, d_dp4 = make_gan()
    pkg.trainers.sync_batchnorm(G4)
    pkg.trainers.sync_batchnorm(D4)
    snap4 = [[t_.clone() for t_ in state(o)] for o in (g_opt4, d_opt4)]
    bn4 = [(m, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for net_ in (G4, D4)
           for m in net_.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    seg4 = pkg.trainers.GraphedSegments(pkg.trainers.srgan_segments(G4, D4, g_opt4, d_opt4, g_dp4, d_dp4), (lr_img, hr_img),
                                        warmup=1)
    n_items = sum(len(pl[0]) for pl in seg4.plan)
    for o, saved in zip((g_opt4, d_opt4), snap4):
        for t_, t0 in zip(state(o), saved):
            t_.copy_(t0)
    for m, rm, rv, nb in bn4:
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
        m.num_batches_tracked.copy_(nb)
    sync_losses_graph = [float(v) for v in seg4(lr_img, hr_img)]
    sync_p_graph, sync_bn_graph = torch.cat([g_opt4.flat.data, d_opt4.flat.data]).cpu(), bn_state(G4, D4)
    res = {"g": g_dp, "p": p_dp, "p_graph": p_graph, "loss": float(dp.allreduce_scalar(loss.detach().clone())),
           "n_sync": n_sync, "n_items": n_items, "sync_losses": sync_losses, "sync_p": sync_p, "sync_bn": sync_bn,
           "sync_losses_graph": sync_losses_graph, "sync_p_graph": sync_p_graph, "sync_bn_graph": sync_bn_graph,
           "g_single": g_single, "n_groups": n_groups, "n_sends": sum(len(r_) for r_ in sends),
           "covered": sorted(rg for r_ in sends for rg in r_), "numel": flat_s.grad.numel(),
           "gan_losses": gan_losses, "gan_losses_graph": gan_losses_graph, "gan_p": gan_p, "gan_p_graph": gan_p_graph}
    if r == 0:  # single-process reference on the full batch
        net1, flat1, opt1 = make()
        step1 = pkg.trainers.l1_step(net1, opt1, None)
        l1 = step1(x.to(dev), t.to(dev))
        res.update(g1=flat1.grad.clone().cpu(), p1=flat1.data.clone().cpu(), loss1=float(l1))
        # ... and the SRGAN step on the global batch of 4 in one process (no DP, plain BatchNorm): what SyncBN must reproduce
        G1, D1, g_opt1, d_opt1, _, _ = make_gan()
        full_lr, full_hr = fill.rand((4, 3, 8, 8), 31).to(dev), fill.rand((4, 3, 32, 32), 32).to(dev)
        l_full = [float(v) for v in pkg.trainers.srgan_step(G1, D1, g_opt1, d_opt1)(full_lr, full_hr)]
        res.update(full_losses=l_full, full_pg=g_opt1.flat.data.clone().cpu(), full_pd=d_opt1.flat.data.clone().cpu(),
                   full_bn=bn_state(G1, D1), n_g=g_opt1.flat.data.numel())
    # (plain numpy payloads: the result file must not depend on how torch.save de-duplicates storages)
    import pickle
    with open(out % r, "wb") as fh:
        pickle.dump({k: (v.detach().cpu().numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}, fh)
    torch.distributed.destroy_process_group()


def _load(path):
    import pickle
    import numpy as np
    with open(path, "rb") as fh:
        d = pickle.load(fh)
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _check(r0, r1):
    assert torch.equal(r0["g"], r1["g"]) and torch.equal(r0["p"], r1["p"])          # replicas stay identical
    scale = r0["g1"].abs().max()
    assert (r0["g"] - r0["g1"]).abs().max() <= 2e-5 * scale                          # mean of shard grads == full-batch grad
    assert (r0["p"] - r0["p1"]).abs().max() <= 1e-5 * r0["p1"].abs().max() + 2e-6   # same Adam step
    assert abs(r0["loss"] - r0["loss1"]) <= 1e-6 * abs(r0["loss1"]) + 1e-7
    assert (r0["p_graph"] - r0["p"]).abs().max() <= 1e-6 * r0["p"].abs().max() + 2e-6  # hipGraph DP step == eager DP step
    # overlapped + bucketed exchange == one all-reduce after everything, bit for bit; the buckets tile the buffer
    assert torch.equal(r0["g"], r0["g_single"]) and torch.equal(r1["g"], r1["g_single"])
    assert r0["n_groups"] >= 4 and r0["n_sends"] >= 2
    pos = 0
    for lo, hi in r0["covered"]:
        assert lo == pos and hi > lo
        pos = hi
    assert pos == r0["numel"]
    # SRGAN under DP: graphs split at the exchanges == eager, replicas identical
    assert torch.equal(r0["gan_p"], r1["gan_p"]) and torch.equal(r0["gan_p_graph"], r1["gan_p_graph"])
    for a, b in zip(sum(r0["gan_losses"], []), sum(r0["gan_losses_graph"], [])):
        assert abs(a - b) <= 1e-4 * abs(a) + 1e-7
    assert (r0["gan_p_graph"] - r0["gan_p"]).abs().max() <= 1e-4 * r0["gan_p"].abs().max()
    # SyncBN: replicas identical; graphs cut at the statistics all-reduces == eager; and the two-rank step == the
    # single-process step on the global batch (losses are means over the global batch: average of the rank losses for
    # the per-sample terms; parameters and BatchNorm running statistics after the step)
    assert r0["n_sync"] >= 5 and r0["n_items"] > 3 * r0["n_sync"]        # (forward + backward cuts per BatchNorm call)
    assert torch.equal(r0["sync_p"], r1["sync_p"]) and torch.equal(r0["sync_p_graph"], r1["sync_p_graph"])
    assert (r0["sync_p_graph"] - r0["sync_p"]).abs().max() <= 1e-5 * r0["sync_p"].abs().max()
    assert (r0["sync_bn_graph"] - r0["sync_bn"]).abs().max() <= 1e-6 * r0["sync_bn"].abs().max()
    for a, b in zip(r0["sync_losses"], r0["sync_losses_graph"]):
        assert abs(a - b) <= 1e-5 * abs(a) + 1e-7
    for k in range(2):   # d_loss, g_loss: mean over ranks of the shard means == global mean (equal shards)
        both = 0.5 * (r0["sync_losses"][k] + r1["sync_losses"][k])
        assert abs(both - r0["full_losses"][k]) <= 1e-4 * abs(r0["full_losses"][k]), (k, both, r0["full_losses"][k])
    assert (r0["sync_bn"] - r0["full_bn"]).abs().max() <= 1e-5 * r0["full_bn"].abs().max()
    n_g = int(r0["n_g"])
    pd, fd = r0["sync_p"][n_g:], r0["full_pd"]
    assert (pd - fd).norm() <= 1e-5 * fd.norm()                              # D: SGD, the update is linear in the gradient
    pg, fg = r0["sync_p"][:n_g], r0["full_pg"]
    assert (pg - fg).norm() <= 1e-3 * fg.norm()                              # G: Adam's first step is +-lr per element



def _free_port():
    """A port the kernel just handed out for 127.0.0.1 (bound, then released): no pid arithmetic that two tests or a
    leftover listener can collide on."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_dp_two_ranks_match_single_process(gpu, tmp_path):
    world, port = 2, _free_port()
    out = str(tmp_path / "dp%d.pt")
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    _check(_load(out % 0), _load(out % 1))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one GPU per rank (>= 2 visible devices)")
def test_dp_two_ranks_rccl(gpu, tmp_path):
    """The same equivalences over RCCL (backend "nccl", one process per GPU, device_id binding, async bucket
    all-reduces behind the grouped weight-gradient launches, graphs split at the exchange)."""
    world, port = 2, _free_port()
    out = str(tmp_path / "rccl%d.pt")
    mp.spawn(_worker, args=(world, port, out, "nccl"), nprocs=world, join=True)
    _check(_load(out % 0), _load(out % 1))


def _rccl_one_rank_worker(_idx, port, out):
    """RCCL itself under the data-parallel step on a ONE-GPU box: a process group of one rank over backend "nccl"
    (communicator init with device_id binding, broadcast, async bucket all-reduces issued between hipGraph replays,
    stream / event ordering of work.wait()) with SRK_DP_FORCE_COMM keeping every collective in the path."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      SRK_DP_FORCE_COMM="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    import time
    import torch.distributed as dist
    import pytorch_super_resolution_model_collection_amd as pkg
    from oracle import fill
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    x, t = fill.rand((16, 3, 32, 32), 1).to(dev), fill.rand((16, 3, 128, 128), 2).to(dev)

    def make(use_dp):
        net = pkg.EDSRNet(3, 64, 4)
        fill.fill_module(net, 7, 0.5)
        net.to(dev).train()
        flat = pkg.optim.FlatParams(net)
        opt = pkg.optim.make_optimizer("edsr", flat, 1e-4)
        dp = pkg.dp.DataParallel(flat, bucket_bytes=256 << 10) if use_dp else None
        if dp is not None:
            assert dp.active and dp.world == 1
            dp.broadcast_params()
        return net, flat, opt, dp

    res = {}
    # eager overlapped exchange, then graphs split at the exchange: both must equal the plain single-GPU step exactly
    # (SUM over one rank is the identity) and no replay may stall
    for name, use_dp, graphed in (("plain", False, False), ("dp_eager", True, False), ("dp_graph", True, True)):
        net, flat, opt, dp = make(use_dp)
        if graphed:
            step = pkg.trainers.GraphedStep(net, opt, pkg.ops.l1_loss, (x, t), dp=dp, warmup=0)
            assert isinstance(step.seg, pkg.trainers.GraphedSegments) and len(step.seg.plan[0][2]) >= 1
        else:
            step = pkg.trainers.l1_step(net, opt, dp)
        times, losses = [], []
        for _ in range(12):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses.append(float(step(x, t).detach()))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res[name] = {"p": flat.data.detach().cpu(), "losses": losses, "times": times}
        if graphed:
            step.close()
    # SRGAN: two models, two exchanges per step, graphs split at both
    G, D = pkg.SRGANGenerator(3, 64, 2), pkg.SRGANDiscriminator(3, 64, 32)
    fill.fill_module(G, 3, 0.5)
    fill.fill_module(D, 4, 0.5)
    G.to(dev).train()
    D.to(dev).train()
    gflat, dflat = pkg.optim.FlatParams(G), pkg.optim.FlatParams(D)
    g_opt, d_opt = pkg.optim.make_optimizer("srgan_g", gflat, 1e-4), pkg.optim.make_optimizer("srgan_d", dflat, 1e-4)
    g_dp, d_dp = pkg.dp.DataParallel(gflat), pkg.dp.DataParallel(dflat)
    lr_img, hr_img = fill.rand((4, 3, 8, 8), 5).to(dev), fill.rand((4, 3, 32, 32), 6).to(dev)
    sstep = pkg.trainers.GraphedSegments(pkg.trainers.srgan_segments(G, D, g_opt, d_opt, g_dp, d_dp), (lr_img, hr_img), warmup=1)
    gan = [[float(v) for v in sstep(lr_img, hr_img)] for _ in range(3)]
    torch.cuda.synchronize()
    res["gan_losses"] = gan
    import pickle
    with open(out, "wb") as fh:
        pickle.dump({k: ({kk: (vv.numpy() if hasattr(vv, "numpy") else vv) for kk, vv in v.items()} if isinstance(v, dict) else v)
                     for k, v in res.items()}, fh)
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_single_rank_under_the_dp_step(gpu, tmp_path):
    """What a one-GPU box can say about RCCL: the collectives of the data-parallel paths (eager overlapped exchange;
    hipGraphs split at the exchange, EDSR and SRGAN) really run on backend "nccl", give the single-GPU result bit for
    bit, and no step hangs behind a collective issued between graph replays."""
    import pickle
    import numpy as np
    out = str(tmp_path / "rccl1.pkl")
    mp.spawn(_rccl_one_rank_worker, args=(_free_port(), out), nprocs=1, join=True)
    with open(out, "rb") as fh:
        r = pickle.load(fh)
    for name in ("dp_eager", "dp_graph"):
        assert np.array_equal(r[name]["p"], r["plain"]["p"]), name
        assert r[name]["losses"] == r["plain"]["losses"], name
        # step-time spread is a RECORD, not a correctness condition (a leased box's jitter must never abort the parity
        # suite): printed with -s / on failure; the only bound is "no replay hung behind a collective" at 30 s
        tt = r[name]["times"]
        print("%s step ms: %s" % (name, " ".join("%.2f" % (1e3 * v) for v in tt)))
        assert max(tt[2:]) < 30.0, (name, tt)
    assert all(np.isfinite(v) for row in r["gan_losses"] for v in row)


def test_bench_runs_its_multi_rank_code_path_on_one_gpu(gpu):
    """bench.py's N > 1 sections (strong- and weak-scaled c4 with the overlapped RCCL exchange, c5 as graphs split at both
    exchanges, the side-metric watchdog, the rank spans) driven end to end on ONE GPU: SRK_DP_FORCE_COMM=1 makes a one-rank
    process group over backend "nccl", so every collective of the data-parallel paths really runs.  The numbers mean nothing;
    the point is that the first real 8-GPU run cannot die on plumbing: rc 0, ONE JSON line on stdout, the N > 1 keys present."""
    import json
    import subprocess
    env = dict(os.environ, SRK_DP_FORCE_COMM="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0", SRK_BENCH_EXTRA_TIMEOUT="600")
    env.pop("SRK_ENV_LIVE", None)     # the product configuration: switches read once
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--full", "--extra-steps", "5", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    ex = rec["extra"]
    assert rec["n_gpus"] == 1 and rec["value"] > 0
    assert ex["rccl_ranks_seen"] == 1 and ex["dist_backend"] == "nccl"
    for key in ("c4_exposed_comm_ms", "c4_ms_per_step_without_exchange", "c4_rank_local_ms_per_step_min_max",
                "c4_weak_ms_per_step", "c4_gradient_bytes_per_step", "c5_srgan_ms_per_step"):
        assert key in ex, (key, sorted(ex))
    assert not [k for k in ex if k.endswith("_error")], {k: v for k, v in ex.items() if k.endswith("_error")}
