"""Data-parallel path with two ranks sharing the one GPU of the test box (gloo transport, CUDA tensors):
SyncBN + bucketed gradient all-reduce must reproduce the single-process step on the concatenated batch.
(RCCL itself needs one GPU per rank; the collective CALL SITES are identical under backend "nccl".)"""
import os
import socket

import numpy as np

import pytest
import torch

pytestmark = pytest.mark.gpu


def _build(seed):
    from object_detection_cib_amd.core.anchors.info import voc_anchor_info
    from object_detection_cib_amd.core.bbox.iou import IoUCalculator
    from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(seed)
    net = Yolov5Network(3, 10, widen_factor=0.25, deepen_factor=0.33).cuda().train()
    asg = Yolov5LabelAssigner(AssignmentAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32)), 4.0)
    return net, Yolov5Loss(asg, Yolov5LossParams.get_default(), IoUCalculator("ciou", 1e-7), None)


def _data(size):
    from oracle import synth
    x, _ = synth.batch(4, size, 10, 3)
    tg = synth.targets(2, size, 10, 3, nmin=6, nmax=12)
    return x, tg + tg          # images 2,3 carry the same boxes as 0,1 => equal per-rank loss normalisers


def _run(net, loss, x, tg, size):
    from object_detection_cib_amd.core.types import FeatureShape
    from object_detection_cib_amd.data.detection import DetectionTarget
    res = net(x.cuda())
    lr = loss(FeatureShape(width=size, height=size), res, tuple(DetectionTarget(b, l) for b, l in tg))
    total = x.shape[0] * (lr.localization + lr.classification + lr.objectness)
    total.backward()
    net.engine().wait_grads()
    return total.item()


def _worker(rank, world, port, size, out, syncbn="rccl"):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["KODHIP_SYNCBN"] = syncbn             # "rccl": collectives of the group (gloo here); "peer": IPC peer buffers
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        net, loss = _build(5)
        net.configure_distributed(None, sync_batchnorm=True, bucket_mb=0.5)
        assert (net.engine().peer is not None) == (syncbn == "peer")
        x, tg = _data(size)
        _run(net, loss, x[2 * rank:2 * rank + 2], tg[2 * rank:2 * rank + 2], size)
        g = torch.cat([p.grad.flatten() for p in net.parameters()]).cpu()
        rm = net.engine().rm_arena.cpu()
        net.engine().sgd_step((0.1, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0), 1.0 / world)
        torch.cuda.synchronize()
        p = torch.cat([q.detach().flatten() for q in net.parameters()]).cpu()
        if net.engine().peer is not None:
            assert not net.engine().peer.timed_out()
            net.engine().peer.close()
        if rank == 0:
            torch.save(dict(g=g, rm=rm, p=p), out)
    finally:
        dist.destroy_process_group()


def test_two_rank_ddp_syncbn_transports_agree_and_equal_single_process(tmp_path):
    """256 px: every layer's per-rank row count (2 images) is then a multiple of the 128-row conv tile, so the fp32
    per-tile statistic partials of the single-process run coincide with the ranks' and only their fp64 combination
    order differs - the forward passes agree bit for bit.  (At 128 px the deepest maps hold 32 rows per rank: the split
    fp32 sums differ in the last ulp, and a single flipped bf16 rounding in this 4-image, random-init, train-mode-BN
    network moves the gradients by 20 % - chaos, not an exchange error; seen when the 3x3 kernels' summation order
    changed.)"""
    import torch.multiprocessing as mp
    size = 256
    ctx = mp.get_context("spawn")
    res = {}
    # SyncBN statistics through the group's collectives, and through IPC-mapped peer buffers (two processes mapping
    # each other's exchange buffer on the one GPU): the two transports must agree bit for bit.
    for mode in ("rccl", "peer"):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        out = str(tmp_path / f"ddp_{mode}.pt")
        procs = [ctx.Process(target=_worker, args=(r, 2, port, size, out, mode)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0, mode
        res[mode] = torch.load(out)
    for k in ("g", "rm", "p"):
        assert torch.equal(res["peer"][k], res["rccl"][k]), k
    # single process on all 4 images against the peer route
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
    got = res["peer"]
    net, loss = _build(5)
    x, tg = _data(size)
    _run(net, loss, x, tg, size)
    g1 = torch.cat([p.grad.flatten() for p in net.parameters()]).cpu()
    # summed DDP gradients = sum of per-rank gradients; single-process total = 4*(...) = 2x each rank's scaling
    assert rel(got["g"], g1) < 2e-2, rel(got["g"], g1)
    assert rel(got["rm"], net.engine().rm_arena.cpu()) < 1e-3
    net.engine().sgd_step((0.1, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0), 0.5)
    p1 = torch.cat([q.detach().flatten() for q in net.parameters()]).cpu()
    assert rel(got["p"], p1) < 1e-4


def _native_worker(port, size, out):
    """One rank, own RCCL communicator (the product transport): raw collectives + a captured training step."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["KODHIP_FORCE_COLLECTIVES"] = "1"          # keep the N>1 code path on a 1-rank group
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        torch.cuda.set_device(0)
        from object_detection_cib_amd.engine.comm import RcclComm
        comm = RcclComm(None, torch.device("cuda", 0))
        a = torch.arange(1000, dtype=torch.float32, device="cuda")
        b = torch.arange(64, dtype=torch.float64, device="cuda") / 3
        a0, b0 = a.clone(), b.clone()
        comm.all_reduce(a); comm.all_reduce(b); comm.broadcast(a, 0)
        torch.cuda.synchronize()
        assert torch.equal(a, a0) and torch.equal(b, b0)
        comm.close()

        x, tg = _data(size)
        res = {}
        for mode in ("plain", "default-eager", "default-graph", "inorder-eager", "inorder-graph", "rccl-eager", "rccl-graph"):
            net, loss = _build(5)
            eng = net.engine()
            if mode.startswith("rccl"):          # SyncBN statistics as RCCL all-reduces instead of the peer exchange (default)
                eng.opt.syncbn_exchange = "rccl"
            # default-*: what a job gets without any switch - gradient buckets overlapped with backward on the
            # weight-gradient stream through their own communicator; inorder-*: KODHIP_COMM_OVERLAP=0
            assert eng.comm_overlap, "bucket / backward overlap must be the default"
            if mode.startswith("inorder"):
                eng.comm_overlap = False
            if mode != "plain":
                net.configure_distributed(None, sync_batchnorm=True, bucket_mb=0.5, native_rccl=True)
                assert eng.comm is not None and eng.collectives
                assert (eng.comm_buckets is not None) == eng.comm_overlap
                assert (eng.peer is not None) == (not mode.startswith("rccl"))
            eng.sgd_step((0.1, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0), 1.0)
            from object_detection_cib_amd.core.label_assignment.yv5 import BatchedTargets
            from object_detection_cib_amd.core.types import FeatureShape
            from object_detection_cib_amd.data.detection import DetectionTarget
            xb = x.cuda()
            bt = BatchedTargets.from_targets(tuple(DetectionTarget(b_, l_) for b_, l_ in tg), torch.device("cuda", 0))
            params = list(net.parameters())

            def step():
                for p in params:
                    p.grad = None
                # Yolov5Network.train_step: the route bench.py and the captured training loop take (label assignment on
                # a side stream, one pass of the loss kernels, engine backward)
                total, _ = net.train_step(xb, loss, FeatureShape(width=size, height=size), bt, 4.0)
                eng.wait_grads()
                eng.sgd_step_device()
                return total
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                losses = [step().item() for _ in range(2)]
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            if mode.endswith("-graph"):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    last = step()
                for _ in range(3):
                    g.replay()
                    losses.append(last.item())
            else:
                losses += [step().item() for _ in range(3)]
            res[mode] = (losses, torch.cat([q.detach().flatten() for q in net.parameters()]).cpu())
            if eng.peer is not None:
                assert not eng.peer.timed_out()
            for c in (eng.comm, eng.comm_buckets, eng.peer):
                if c is not None:
                    c.close()
        torch.save(res, out)
    finally:
        dist.destroy_process_group()


def test_native_rccl_comm_and_captured_step(tmp_path):
    """The RCCL transport of the product path on the single GPU of the test box: a 1-rank communicator must be an
    identity, and a training step with SyncBN sums + gradient buckets going through it - eagerly and replayed as
    one hipGraph - must reproduce the plain single-GPU trajectory bit for bit."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "native.pt")
    p = mp.get_context("spawn").Process(target=_native_worker, args=(port, 128, out))
    p.start()
    p.join(300)
    assert p.exitcode == 0
    res = torch.load(out)
    ref_l, ref_p = res["plain"]
    # default-*: gradient buckets on the weight-gradient stream through their own communicator, eager and captured;
    # inorder-*: every collective on the main stream (KODHIP_COMM_OVERLAP=0)
    # rccl-*: SyncBN statistics as RCCL all-reduces (KODHIP_SYNCBN=rccl) instead of the peer-buffer exchange
    for mode in ("default-eager", "default-graph", "inorder-eager", "inorder-graph", "rccl-eager", "rccl-graph"):
        l, prm = res[mode]
        assert l == ref_l, (mode, l, ref_l)
        assert torch.equal(prm, ref_p), mode


def test_bench_self_launch_runs_the_collective_path():
    """`python bench.py --gpus N` with WORLD_SIZE unset (the driver's plain command) starts the ranks itself.  Rehearsed
    here with one rank and KODHIP_FORCE_COLLECTIVES=1: a fresh child process, its own RCCL communicators, SyncBN sums +
    gradient buckets (overlapped with backward, the default) inside the replayed hipGraph; ONE JSON line comes back
    (--full: with the family table and the training-loop leg, which run the collective path too)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["KODHIP_FORCE_COLLECTIVES"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--launch", "self", "--steps", "3",
                        "--warmup", "2", "--batch", "8", "--size", "320", "--full", "--no-cpu-baseline", "--timeout", "400"],
                       capture_output=True, text=True, timeout=500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and len(d["per_rank_images_per_sec"]) == 1
    cfg = d["config"]
    assert cfg["launcher"] == "self" and cfg["launch"] == "hipGraph replay", cfg
    assert "RCCL" in cfg["collectives"] and "overlapped with backward" in cfg["collectives"], cfg
    assert d["engine_options"]["comm_overlap"] is True and d["engine_options"]["force_collectives"] is True
    assert abs(sum(f["share_of_step"] for f in d["families"]) - 1.0) < 0.02
    # the training-loop leg runs on the collective path too (every rank with its own producer process, mixup on: configs[2])
    assert d["loop"]["value"] > 0 and "producer process" in d["loop"]["workload"] and "mixup p=0.1" not in d["loop"]["workload"]
    assert d["loop"]["per_rank_ms_per_step"] == [d["loop"]["ms_per_step"]]


@pytest.mark.parametrize("ranks,batch,size", [(2, 4, 256), (4, 2, 128)])
def test_bench_ranks_on_one_gpu_control_flow(ranks, batch, size):
    """`python bench.py --gpus N` end to end on the one GPU of the test box (KODHIP_BENCH_ONE_GPU=1): the parent starts N
    fresh ranks, they rendezvous, map each other's SyncBN exchange buffer through HIP IPC (N = 4: twelve mappings, lanes
    4r .. 4r + 3 for r < 4 - the box allows six GPU processes, so this is as wide as real IPC gets here; the full eight-rank
    width is the one-process test below), train with bucketed gradient all-reduces (through the gloo group here: RCCL wants
    one GPU per rank) and rank 0 reports ONE line for the job with every rank's rate.  What an 8-GPU run adds to this is RCCL
    and xGMI, not control flow."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["KODHIP_BENCH_ONE_GPU"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--steps", "3", "--warmup", "2",
                        "--batch", str(batch), "--size", str(size), "--no-cpu-baseline", "--timeout", "400"],
                       capture_output=True, text=True, timeout=500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == ranks and d["config"]["global_batch"] == ranks * batch and len(d["per_rank_images_per_sec"]) == ranks
    assert d["config"]["launcher"] == "self" and d["config"]["parallelism"] == f"dp{ranks}+syncbn"
    assert "IPC peer buffers" in d["config"]["collectives"], d["config"]
    assert d["engine_options"]["syncbn_exchange"] == "peer"
    assert abs(d["value"] - ranks * batch * 3 / (3 * d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]      # whole-job rate over all ranks
    assert np.isfinite(d["final_loss"])


def test_peer_exchange_eight_ranks_in_one_process_and_desync_detection():
    """The SyncBN statistic exchange at its full width (kodhip_peer_*, csrc/bn_act.hip peer_allreduce2: lanes 4r .. 4r + 3
    poll rank r, r < 8) - on the one GPU of the test box as EIGHT exchange buffers in one process, connected through
    kodhip_peer_connect_local (the box allows at most six GPU processes, so eight IPC-mapped ranks cannot run here; the
    kernels do not know the difference: they see eight granule areas).  (1) three rounds of rank-dependent random fp64
    vectors: every rank gets the rank-order sum, bit for bit, no verdict raised; (2) a rank whose step counter ran ahead
    (one extra kodhip_peer_step_begin: an uneven number of training forwards) is detected: no rank folds a stale payload
    into its sums - the results are NaN - and the verdict (1: a poll gave up, 2: step counters diverged) is readable from
    the pinned host mirror without synchronising (kodhip_peer_status)."""
    import ctypes as C
    from object_detection_cib_amd import _lib
    lib, chk = _lib.lib(), _lib.check
    world, n, gran = 8, 600, 4096
    handles = []
    for r in range(world):
        h = C.c_void_p()
        chk(lib.kodhip_peer_create(C.byref(h), r, world, gran), "peer_create")
        handles.append(h)
    arr = (C.c_void_p * world)(*[h.value for h in handles])
    s0 = torch.cuda.current_stream().cuda_stream
    try:
        for h in handles:
            chk(lib.kodhip_peer_connect_local(h, arr), "peer_connect_local")
        torch.cuda.synchronize()

        def exchange(k, extra_begin=()):
            srcs = [torch.randn(n, generator=torch.Generator().manual_seed(100 * k + r), dtype=torch.float64) for r in range(world)]
            dev = [s.cuda() for s in srcs]
            outs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(world)]
            for r in list(extra_begin) + list(range(world)):
                chk(lib.kodhip_peer_step_begin(handles[r], s0), "step_begin")
            # all eight ranks' exchange kernels as ONE dispatch (blockIdx.y = rank): co-resident by construction - eight
            # polling launches on eight streams would share the process's four hardware queues
            ins_a = (C.c_void_p * world)(*[d.data_ptr() for d in dev])
            outs_a = (C.c_void_p * world)(*[o.data_ptr() for o in outs])
            chk(lib.kodhip_peer_allreduce_f64_multi(arr, world, ins_a, outs_a, n, 16 * k, s0), "allreduce_multi")
            torch.cuda.synchronize()
            want = srcs[0].clone()
            for s in srcs[1:]:
                want += s                      # rank order, like the kernel
            return [o.cpu() for o in outs], want

        def status(r):
            f = C.c_int(0)
            chk(lib.kodhip_peer_status(handles[r], C.byref(f)), "peer_status")
            return f.value
        for k in range(3):
            outs, want = exchange(k)
            for r in range(world):
                assert torch.equal(outs[r], want), (k, r)
                assert status(r) == 0
        outs, _ = exchange(3, extra_begin=(3,))          # rank 3 is one step ahead from here on
        verdicts = [status(r) for r in range(world)]
        assert all(v == 2 for v in verdicts), verdicts          # (nobody had to wait for a time-out to find out)
        for r in range(world):
            assert torch.isnan(outs[r]).all(), r          # never a stale or partial sum
        for r in range(world):                            # the synchronising read reports the same verdict and resets it
            f = C.c_int(0)
            chk(lib.kodhip_peer_timed_out(handles[r], C.byref(f)), "peer_timed_out")
            assert f.value == verdicts[r] and status(r) == 0
    finally:
        torch.cuda.synchronize()
        for h in handles:
            lib.kodhip_peer_destroy(h)


def _oracle_ddp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["KODHIP_SYNCBN"] = "peer"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import synth
        from object_detection_cib_amd.core.anchors.info import voc_anchor_info
        from object_detection_cib_amd.core.bbox.iou import IoUCalculator
        from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo
        from object_detection_cib_amd.core.types import FeatureShape
        from object_detection_cib_amd.data.detection import DetectionTarget
        from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams
        from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
        torch.cuda.set_device(0)
        nc, B, size, seed = 10, 16, 640, 2023
        torch.manual_seed(seed)
        net = Yolov5Network(3, nc, widen_factor=0.5, deepen_factor=0.33).cuda().train()
        asg = Yolov5LabelAssigner(AssignmentAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32)), 4.0)
        loss = Yolov5Loss(asg, Yolov5LossParams.get_default(), IoUCalculator("ciou", 1e-7), None)
        net.configure_distributed(None, sync_batchnorm=True, bucket_mb=8.0)
        assert net.engine().peer is not None
        x, tg = synth.batch(B, size, nc, seed)
        per = B // world
        xs, tgs = x[rank * per:(rank + 1) * per], tg[rank * per:(rank + 1) * per]
        res = net(xs.cuda())
        lr = loss(FeatureShape(width=size, height=size), res, tuple(DetectionTarget(b, l) for b, l in tgs))
        total = per * (lr.localization + lr.classification + lr.objectness)       # exp.py:104-138 on this rank's batch
        total.backward()
        net.engine().wait_grads()
        torch.cuda.synchronize()
        assert not net.engine().peer.timed_out()
        mine = [lr.localization.item(), lr.objectness.item(), lr.classification.item(), total.item()]
        every = [None] * world
        dist.all_gather_object(every, mine)
        if rank == 0:
            torch.save(dict(losses=every, grads={k: p.grad.detach().cpu() for k, p in net.named_parameters()},
                            state={k: v.detach().cpu() for k, v in net.state_dict().items() if "running" in k}), out)
        net.engine().peer.close()
    finally:
        dist.destroy_process_group()


def test_two_rank_ddp_syncbn_vs_fp32_oracle(tmp_path):
    """a23 against the ORACLE (not against another HIP run): two data-parallel ranks - SyncBN statistics over the peer
    buffers, gradient buckets summed over the group - on the two halves of a 16-image batch at 640 px, compared with the
    fp32 CPU oracle (pinned to the reference) doing what Lightning's DDP + `sync_batchnorm: True` does
    (kod/configs/trainer/ddp.yaml:4-9): ONE forward of the whole batch in train mode (SyncBatchNorm = batch statistics over
    all ranks' pixels), each rank's loss normalised by that rank's own counts and scaled by its own batch size
    (kod/lightning/experiments/yv5_baseline/loss.py:96,120-124, exp.py:104-138), gradients summed over ranks.  Same bars as
    test_train_step_well_conditioned_batch: every rank's losses <= 1e-2, global gradient norm <= 5e-2, per-tensor cosine
    against fp32 no further off than the oracle's own bf16-storage emulation (- 0.15), BatchNorm running statistics."""
    import torch.multiprocessing as mp
    from oracle import bf16_emul, detection as D, synth
    from oracle.network import OracleYolov5, HeadOut, NetOut
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "ddp_oracle.pt")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_oracle_ddp_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    nc, B, size, seed = 10, 16, 640, 2023
    x, tg = synth.batch(B, size, nc, seed)
    per = B // world

    def oracle_step(model):
        o = model(x)
        totals, parts = 0.0, []
        for r in range(world):
            sl = slice(r * per, (r + 1) * per)
            lr = D.yolo_loss(size, size, NetOut(*[HeadOut(h.box[sl], h.obj[sl], h.cls[sl]) for h in o]),
                             [D.Target(b, l) for b, l in tg[sl]])
            t = D.train_step_total(lr, per)
            parts.append([lr.localization.item(), lr.objectness.item(), lr.classification.item(), t.item()])
            totals = totals + t
        totals.backward()
        return parts
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, 0.5, 0.33).train()
    torch.manual_seed(seed)
    emu = bf16_emul.emulate(OracleYolov5(3, nc, 0.5, 0.33).train())
    want = oracle_step(ref)             # (runs while the two ranks do their step)
    oracle_step(emu)
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = torch.load(out)
    np.testing.assert_allclose(np.array(got["losses"]), np.array(want), rtol=1e-2)
    gr = {k: p.grad.double() for k, p in ref.named_parameters()}
    ge = {k: p.grad.double() for k, p in emu.named_parameters()}
    gh = {k: v.double() for k, v in got["grads"].items()}
    gn_r = torch.sqrt(sum((g ** 2).sum() for g in gr.values())).item()
    gn_h = torch.sqrt(sum((g ** 2).sum() for g in gh.values())).item()
    assert abs(gn_h - gn_r) <= 5e-2 * gn_r, (gn_h, gn_r)
    cos = lambda a, b: (a.flatten() @ b.flatten() / (a.norm() * b.norm() + 1e-300)).item()
    rows = [(k, cos(gh[k], g), cos(ge[k], g)) for k, g in gr.items() if g.norm().item() >= 1e-3 * gn_r]
    ch, ce = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    worst = min(rows, key=lambda r: r[1] - r[2])
    print(f"two ranks vs the fp32 oracle: grad norm HIP {gn_h:.4f} vs oracle {gn_r:.4f}; {len(rows)} tensors; cosine vs fp32: HIP median "
          f"{np.median(ch):.4f} min {ch.min():.4f} | bf16-emulated oracle median {np.median(ce):.4f} min {ce.min():.4f}; largest deficit "
          f"{worst[1] - worst[2]:+.4f} at {worst[0]}")
    assert len(rows) >= 100
    assert (ch >= ce - 0.15).all(), worst
    assert abs(np.median(ch) - np.median(ce)) <= 0.03 and np.abs(ch - ce).mean() <= 0.05
    rel = lambda a, b: ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    sd_r = ref.state_dict()
    for suffix, tol in (("running_mean", 2e-2), ("running_var", 5e-3)):
        a = torch.cat([got["state"][k].flatten() for k in sd_r if k.endswith(suffix)])
        b = torch.cat([sd_r[k].flatten() for k in sd_r if k.endswith(suffix)])
        assert rel(a, b) <= tol, (suffix, rel(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("die_rank", [None, 1, "hang"])
def test_bench_under_torch_distributed_run_and_attempt_ladder(die_rank):
    """The driver's own N > 1 command - `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py --gpus N ...` - on the one GPU of the test box (KODHIP_BENCH_ONE_GPU=1, two ranks):
    the launcher's processes supervise, their children are the ranks (launcher's env contract, agent store rendezvous),
    rank 0 prints the job's one line.  With a rank that dies in attempt 0 (test hook) every supervisor stops its child and
    the job runs again on the next rung of bench.ATTEMPTS; the line then says which attempt produced it, carries
    "degraded": true and what ended the earlier attempt (a crash and a stall are told apart), and the job's exit code is
    non-zero unless --allow-fallback was given.  The same when a
    rank hangs: no rank reaches a new phase (heartbeat files, bench._beat) for STALL_S seconds."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                             "KODHIP_BENCH_LAUNCHER", "KODHIP_BENCH_ATTEMPT")}
    env["KODHIP_BENCH_ONE_GPU"] = "1"
    if die_rank == "hang":          # rank 1 stops making progress: no rank reaches a new phase -> stall verdict, next attempt
        env["KODHIP_BENCH_TEST_HANG_RANK"], env["KODHIP_BENCH_STALL_S"] = "1", "25"
    elif die_rank is not None:
        env["KODHIP_BENCH_TEST_DIE_RANK"] = str(die_rank)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                        "--gpus", "2", "--steps", "3", "--warmup", "2", "--batch", "4", "--size", "256", "--no-cpu-baseline",
                        "--timeout", "300"] + (["--allow-fallback"] if die_rank == "hang" else []),
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    # a result measured down the ladder is not a successful run of the job as asked: the supervisors exit EXIT_DEGRADED (the
    # launcher then reports failure) unless --allow-fallback was given; the line itself is printed either way and says so
    if die_rank == 1:
        assert r.returncode != 0, "a degraded result must not look like a successful scaling run"
    else:
        assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["launcher"] == "external" and len(d["per_rank_images_per_sec"]) == 2
    assert d["config"]["attempt"] == (0 if die_rank is None else 1)
    assert d["degraded"] is (die_rank is not None)
    if die_rank is not None:
        assert "attempt 0" in r.stderr and d["config"]["fallback"] == {"KODHIP_BENCH_NO_GRAPH": "1"}
        assert ("stalled" if die_rank == "hang" else "crashed") in d["earlier_attempts"]
    else:
        assert d["earlier_attempts"] is None
    assert np.isfinite(d["final_loss"])


@pytest.mark.gpu
def test_bench_ranks_die_with_their_launcher():
    """A launcher that gives up (the driver's timeout) signals ITS children - bench.py's supervisors - not theirs: the
    supervisors take their ranks along on SIGTERM, and a rank whose supervisor was killed outright gets SIGKILL through
    PR_SET_PDEATHSIG, so nothing keeps the GPU busy under the next run.  Here: a two-rank job whose rank 1 hangs (test
    hook) is started under torch.distributed.run, the launcher is terminated, and no process of the job (found by a
    marker in its environment) is left."""
    import signal
    import subprocess
    import sys
    import time
    import uuid
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    tag = "kodtag_" + uuid.uuid4().hex
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                             "KODHIP_BENCH_LAUNCHER", "KODHIP_BENCH_ATTEMPT")}
    env.update(KODHIP_BENCH_ONE_GPU="1", KODHIP_BENCH_TEST_HANG_RANK="1", KODHIP_BENCH_STALL_S="600", KODHIP_TEST_MARK=tag)

    def alive():
        pids = []
        for d in os.listdir("/proc"):
            if d.isdigit() and int(d) != os.getpid():
                try:
                    with open(f"/proc/{d}/environ", "rb") as f:
                        if tag.encode() in f.read():
                            pids.append(int(d))
                except OSError:
                    pass
        return pids
    p = subprocess.Popen([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                          "--gpus", "2", "--steps", "3", "--warmup", "2", "--batch", "4", "--size", "256", "--no-cpu-baseline",
                          "--timeout", "600"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=env, cwd=root)
    try:
        deadline = time.time() + 120
        while len(alive()) < 5 and time.time() < deadline:          # launcher + 2 supervisors + 2 ranks (+ producers later)
            time.sleep(0.5)
        assert len(alive()) >= 5, alive()
        time.sleep(5)
        p.send_signal(signal.SIGTERM)                                # exactly the launcher this test started
        p.wait(60)
        deadline = time.time() + 30
        while alive() and time.time() < deadline:
            time.sleep(0.5)
        assert alive() == [], alive()
    finally:
        if p.poll() is None:
            p.kill()
