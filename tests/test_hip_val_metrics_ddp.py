"""DeviceDetectionMetrics.gather over two ranks (gloo, both on GPU 0): rank r is fed half r of a 16-image batch; after the
gather every rank holds the whole batch's records in rank order - the state of one evaluator fed everything - and computes the
same bits.  A rank that was never fed takes part too."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import val_metrics_reference as R  # noqa: E402


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from object_detection_cib_amd.data.detection import DetectionTarget
        from object_detection_cib_amd.lightning.callbacks.val_metrics import DeviceDetectionMetrics
        case = R.random_batch(5, 51)

        def feed(vm, sl):
            tg = tuple(DetectionTarget(torch.from_numpy(np.asarray(g, np.float64).reshape(-1, 4)), torch.from_numpy(np.asarray(l, np.int64)))
                       for g, l in case.gts[sl])
            vm.add_batch(tg, [torch.from_numpy(d).cuda() for d in case.dets[sl]])

        vm = DeviceDetectionMetrics(5, initial_capacity=128)
        feed(vm, slice(0, 8) if rank == 0 else slice(8, 16))
        assert vm.gather(dist.group.WORLD) is vm
        state = (*vm.records(), vm.ground_truths())
        cur = vm.curves()
        lone = DeviceDetectionMetrics(5)                       # rank 1 was never fed: its peers' records arrive all the same
        if rank == 0:
            feed(lone, slice(0, 16))
        res = lone.compute(dist.group.WORLD)
        q.put((rank, [np.asarray(a) for a in state], {k: cur[k] for k in ("p", "r", "ap", "n_p", "nt")},
               (res["map"], res["best_conf"], int(res["n_p"].sum()))))
    finally:
        dist.destroy_process_group()


def test_gather_gives_every_rank_the_whole_set_in_rank_order():
    case = R.random_batch(5, 51)
    want = R.process(case.dets, case.gts, 5, case.thrs)
    ref = R.curves_ref(*want, 5, 10)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(60)
    assert [r[0] for r in res] == [0, 1]
    for rank, state, cur, lone in res:
        for g, w, what in zip(state, want, ("scores", "classes", "masks", "nt")):
            np.testing.assert_array_equal(g, w, err_msg=f"rank {rank} {what}")
        np.testing.assert_array_equal(cur["n_p"], ref["n_p"])
        for k in ("p", "r", "ap"):
            assert np.abs(cur[k] - ref[k]).max() <= 1e-12, (rank, k)
        assert lone[2] == len(want[0])
    for k in res[0][2]:
        np.testing.assert_array_equal(res[0][2][k], res[1][2][k], err_msg=k)          # identical state -> identical bits
    assert res[0][3] == res[1][3]
