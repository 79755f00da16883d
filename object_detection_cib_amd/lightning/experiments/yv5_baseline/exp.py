"""DefaultYolov5Experiment without Lightning: the arithmetic and call order of
kod/lightning/experiments/yv5_baseline/exp.py:36-185 (training_step, validation_step, configure_optimizers,
on_before_optimizer_step) plus the epoch loop Lightning's Trainer.fit provides (automatic optimisation:
zero_grad -> backward -> warm-up hook -> optimizer.step; LambdaLR.step per epoch).  `lightning` is not
installed in the target image; a LightningModule shell can wrap these methods one to one.
"""
from __future__ import annotations

import contextlib
import gc
from functools import partial
from typing import Callable, Optional, Sequence

import torch

from .... import _lib
from ....core.types import FeatureShape
from ....core.nms import non_max_suppression
from ....core.label_assignment.yv5 import BatchedTargets
from ....nn.optim.smart import SmartOptimizer, FusedSGD, FusedAdam, CLIP_ALGORITHMS
from ....nn.optim.schedulers import LinearScheduler
from ...callbacks.map_eval import DeviceMAPEvaluator
from .layers import get_detections, get_detections_augmented
from .type_defs import LayerwiseAnchorInfo
from .warmup import OptimizerWarmupUpdater


@contextlib.contextmanager
def _gc_paused():
    """The epoch loops run at ~10 ms per batch; a generation-2 collection of the interpreter (triggered every few
    batches by the many small host objects a batch creates) walks the whole heap and stalls the loop for 60-80 ms -
    measured: validation 32 ms/batch with the collector on, 10 ms with it paused.  Collect once, before and after."""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()
        gc.collect()            # reference cycles built while paused (they may hold device tensors) go now


class DefaultYolov5Experiment:
    """Constructor = the reference's (exp.py:37-58: net, loss, anchor_info, smart_optimizer, lr_scheduler,
    optimizer_warmup_updater, val_nms_conf_threshold, val_nms_iou_threshold); the keyword-only extras stand in for
    what Lightning's Trainer supplies (`trainer.max_epochs`) or are build-side switches.  smart_optimizer /
    lr_scheduler default to the reference's configs (configs/nn/optimizers/smart_sgd.yaml, schedulers/linear.yaml).
    smart_optimizer over torch.optim.SGD, Adam or AdamW: with the HIP network the optimizer is FusedSGD / FusedAdam / FusedAdamW
    (nn/optim/smart.py) and every route below - eager, graphed, multi-scale, EMA, clipping - runs its fused update.
    val_augment=True: validation_step runs YOLOv5's test-time augmentation (val.py --augment) - three views of the batch, one
    NMS over the merged predictions.  The merged tensor has 45147 rows at 640 px against 25200, so the NMS key workspace
    roughly doubles: at nc = 80, 45147 * 80 keys need a 4 Mi-key capacity per image, against 2 Mi without it.
    val_max_graphs: with graphed=True validation_step keeps one captured forward per input shape, at most this many, least
    recently used first (engine/graphed.GraphCache) - rectangular validation batches (DeviceValPipeline.rect_batches +
    make_batch(canvas=...)) bring one shape per canvas; a shape beyond the bound costs a buffer-set allocation and a capture
    again when it comes back.
    multi_scale=True: YOLOv5's train.py --multi-scale - every training batch is resized on the device to a random multiple of
    32 between multi_scale_range[0] and [1] times its size, a new size every multi_scale_interval steps, boxes scaled with it
    (engine/multiscale.py, one kodhip_multiscale_batch launch per step); validation stays at the size of its batches.
    graphed=True keeps one captured step and one engine buffer set per size, at most multi_scale_max_graphs (None: all),
    least recently used first: when the 21 sizes of a 640 px plan do not fit in device memory, narrow multi_scale_range,
    bound multi_scale_max_graphs, and raise multi_scale_interval so that re-captures come less often.  Data parallel: every
    rank must use the same multi_scale_seed (the ranks then draw the same sizes, which SyncBN needs).
    ema=True: YOLOv5's ModelEMA (engine/ema.py) - an exponential moving average of parameters and BatchNorm running statistics
    with decay ema_decay * (1 - exp(-updates / ema_tau)), built with the optimizer and readable as `self.ema`.  optimize() calls
    `ema.update()` after every optimizer step - one kodhip_ema_update launch behind the step, outside any captured graph - and
    validate() runs under `ema.applied()`, i.e. reports the averaged model as train.py does; the network's own weights are
    back, bit for bit, when it returns.  Data parallel: every rank forms the same parameter average without a collective;
    without SyncBN the running statistics and their averages are per rank.
    accumulate_grad_batches=N: Lightning's Trainer argument (YOLOv5's `accumulate`; engine/accumulate.py has train.py's recipe
    as `yolov5_accumulate`).  Every micro-batch runs forward, loss and backward at the scale B / N - `total` is that scaled
    value, the logged box / obj / cls stay unscaled - and moves the BatchNorm running statistics; warm-up, clipping, the update,
    `global_step`, `optimizer.steps_taken` and `ema.update()` happen once per window of N, on the summed gradient.  The last
    batch of an epoch closes the window even when it is partial (fit_epoch does; by hand: step_accumulated()).  graphed=True:
    the captured step ends with one kodhip_grad_accumulate launch and the update runs behind the replay that closes a window;
    eager: the gradients accumulate in `.grad`.  Data parallel: every micro-batch all-reduces its gradients as today and the
    all-reduced gradient is accumulated; Lightning's `no_sync` (one all-reduce per window) is not implemented.  Checkpoints
    belong at window boundaries: the accumulator is not part of a checkpoint."""

    def __init__(self, net, loss, anchor_info: LayerwiseAnchorInfo, smart_optimizer: Optional[SmartOptimizer] = None,
                 lr_scheduler: Optional[Callable] = None,
                 optimizer_warmup_updater: Optional[OptimizerWarmupUpdater] = None,
                 val_nms_conf_threshold: float = 0.001, val_nms_iou_threshold: float = 0.6, *, max_epochs: int = 300,
                 graphed: bool = False, max_targets: int = 4096, world_size: int = 1,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 eval_fused: Optional[bool] = None, val_confusion: bool = False, val_confusion_conf: float = 0.25,
                 val_confusion_iou: float = 0.45, val_augment: bool = False, val_metrics: bool = False,
                 val_max_graphs: int = 8, multi_scale: bool = False, multi_scale_range=(0.5, 1.5),
                 multi_scale_interval: int = 1, multi_scale_max_graphs: Optional[int] = None, multi_scale_seed: int = 0,
                 ema: bool = False, ema_decay: float = 0.9999, ema_tau: float = 2000.0, accumulate_grad_batches: int = 1):
        if gradient_clip_algorithm not in CLIP_ALGORITHMS:
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: expected one of {CLIP_ALGORITHMS}")
        # Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm): handed to the FusedSGD / the captured step
        self.gradient_clip_val, self.gradient_clip_algorithm = gradient_clip_val, gradient_clip_algorithm
        self.net, self.loss, self.anchor_info = net, loss, anchor_info
        self.smart_optimizer = smart_optimizer or SmartOptimizer(
            partial(torch.optim.SGD, lr=0.01, momentum=0.937, nesterov=True), weight_decay=0.0005)
        self.lr_scheduler = lr_scheduler or partial(LinearScheduler, lrf=0.01)
        self.max_epochs = max_epochs
        self.optimizer_warmup_updater = optimizer_warmup_updater
        self.val_nms_conf_threshold = val_nms_conf_threshold
        self.val_nms_iou_threshold = val_nms_iou_threshold
        self.global_step = 0
        self.current_epoch = 0
        self.logged = {}
        self.world_size = world_size
        self.optimizer = self.scheduler = None
        # graphed=True: the optimisation step is captured once as a hipGraph (engine/graphed.py) and replayed - same
        # arithmetic, no per-launch Python; batches must keep one shape and at most max_targets boxes
        self.graphed, self.max_targets, self._gstep = graphed, max_targets, None
        # input shape -> GraphedEvalForward, at most val_max_graphs of them, least recently used first (rectangular
        # validation batches bring one shape per canvas; a shape beyond the bound is captured again when it comes back)
        from ....engine.graphed import GraphCache
        self._geval = GraphCache(val_max_graphs)
        # validation forwards with BatchNorm + activation in the conv epilogue (Yolov5Network.fuse_eval); None leaves the
        # engine's option (EngineOptions.eval_fused / KODHIP_EVAL_FUSED) alone
        self.eval_fused = eval_fused
        # cross-rank validation: "auto" (default) = the group the network was made data-parallel over
        # (Yolov5Network.configure_distributed) with sync "mean", i.e. what the reference logs under DDP
        # (`log_dict(results, sync_dist=True)`, pycoco_map_eval.py:139-142); without such a group every rank reports its
        # own shard.  None = never a collective (rank-0-only validation cannot hang on its peers); an explicit process
        # group + "mean" / "global" = DeviceMAPEvaluator.get_report's two DDP modes
        self.val_process_group, self.val_sync = "auto", "mean"
        # val_confusion: validate() also feeds every batch to a DeviceConfusionMatrix (YOLOv5's val.py diagnostic: the NMS
        # output at the validation thresholds, filtered again at val_confusion_conf inside the kernel) and reports
        # precision_<class> / recall_<class>; the object stays readable as `self.confusion`.  Its counts are SUMMED over
        # the validation group, whatever val_sync says.
        self.val_confusion, self.val_confusion_conf, self.val_confusion_iou = val_confusion, val_confusion_conf, val_confusion_iou
        self.confusion = None
        # val_augment: the forward of validation_step becomes layers.get_detections_augmented (graphed: GraphedAugmentedForward, one
        # hipGraph over all three views); validate(), the mAP evaluator and val_confusion receive the NMS output as without it
        self.val_augment = bool(val_augment)
        # val_metrics: validate() also feeds every batch to a DeviceDetectionMetrics (YOLOv5's val.py table: process_batch +
        # ap_per_class on the device) and reports metrics/precision, metrics/recall, metrics/f1, metrics/best_conf,
        # metrics/mAP_0.5 and metrics/mAP_0.5:0.95; the object stays readable as `self.metrics`.  Under a validation group its
        # records are GATHERED (the whole validation set's values), whatever val_sync says.
        self.val_metrics = bool(val_metrics)
        self.metrics = None
        # multi_scale: the size schedule lives in the captured wrapper (graphed) or in `_ms_schedule` (eager), both built
        # with the first batch; a state loaded before that waits in `_ms_pending`
        self.multi_scale = bool(multi_scale)
        self.multi_scale_range, self.multi_scale_interval = tuple(multi_scale_range), int(multi_scale_interval)
        self.multi_scale_max_graphs, self.multi_scale_seed = multi_scale_max_graphs, int(multi_scale_seed)
        self._ms_schedule, self._ms_pending, self._ms_pairs = None, None, {}
        # ema: the ModelEMA is built with the optimizer (configure_optimizers); a state loaded before that waits in `_ema_pending`
        self._ema_on, self.ema_decay, self.ema_tau = bool(ema), float(ema_decay), float(ema_tau)
        self.ema, self._ema_pending = None, None
        # accumulate_grad_batches: the eager route's window (the graphed one lives in the engine, engine/graphed.py)
        from ....engine.accumulate import AccumulationWindow
        self._window = AccumulationWindow(accumulate_grad_batches)
        self.accumulate_grad_batches = self._window.n
        self._num_training_batches = None

    # exp.py:156-162
    def configure_optimizers(self):
        if self.optimizer is None:
            self.optimizer = self.smart_optimizer(self.net)
            if isinstance(self.optimizer, (FusedSGD, FusedAdam)):
                self.optimizer.world_size = self.world_size
                if self.gradient_clip_val is not None:
                    # (the reference's partial(torch.optim.SGD, ...) knows no such keywords; a partial(FusedSGD, ...) that
                    # carries its own keeps them when the experiment has none)
                    self.optimizer.gradient_clip_val = self.gradient_clip_val
                    self.optimizer.gradient_clip_algorithm = self.gradient_clip_algorithm
                    self.optimizer.track_grad_norm = True          # the grad_norm metric, also under "value"
            elif self.gradient_clip_val is not None and self.graphed:
                raise RuntimeError("gradient_clip_val with graphed=True needs the HIP network's FusedSGD / FusedAdam")
            self.scheduler = self.lr_scheduler(optimizer=self.optimizer, max_epochs=self.max_epochs)
            if self._ema_on:
                from ....engine.ema import ModelEMA
                self.ema = ModelEMA(self.net, self.ema_decay, self.ema_tau)
                if self._ema_pending is not None:
                    self.ema.load_ema_state_dict(self._ema_pending)
                    self._ema_pending = None
        return [self.optimizer], [self.scheduler]

    @property
    def sch_fn(self):
        self.configure_optimizers()
        return self.scheduler.sch_fn

    def _clipping(self) -> bool:
        opt = self.optimizer
        return (self.gradient_clip_val is not None
                or (isinstance(opt, (FusedSGD, FusedAdam)) and (opt.gradient_clip_val is not None or opt.track_grad_norm)))

    def get_metrics_to_display(self):
        return ["box", "cls", "obj"] + (["grad_norm"] if self._clipping() else [])

    # exp.py:104-138
    def training_step(self, batch, batch_idx: int = 0):
        images, targets, _ = batch
        net_result = self.net(images)
        shape = FeatureShape(width=images.shape[3], height=images.shape[2])
        lr = self.loss(shape, net_result, targets)
        B = images.shape[0]
        # accumulate_grad_batches = N: Lightning's loss / N, formed as ONE fp32 factor B / N (total / N afterwards would round twice)
        N = self.accumulate_grad_batches
        total = (B if N == 1 else B / N) * (lr.localization + lr.classification + lr.objectness)
        self.logged = {"obj": lr.objectness.detach(), "cls": lr.classification.detach(), "box": lr.localization.detach()}
        return total

    # exp.py:140-154
    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int = 0):
        images, targets, _ = batch
        if self.graphed:          # eval forward + decode replayed as one hipGraph per input shape (engine/graphed.py)
            from ....engine.graphed import GraphedAugmentedForward, GraphedEvalForward
            key = tuple(images.shape)
            cls = GraphedAugmentedForward if self.val_augment else GraphedEvalForward
            gf = self._geval.forward(key, lambda: cls(self.net, self.anchor_info, key[0], key[2], key[3]))
            det = gf(images if images.dtype == torch.float32 else images.float())
            return targets, non_max_suppression(det, self.val_nms_conf_threshold, self.val_nms_iou_threshold)
        if self.val_augment:      # (the engine's eval forward, called directly: no module mode is touched)
            x = (images if images.dtype == torch.float32 else images.float()).contiguous()
            det = get_detections_augmented(x, self.net, self.anchor_info)
            return targets, non_max_suppression(det, self.val_nms_conf_threshold, self.val_nms_iou_threshold)
        # every submodule's own mode is restored afterwards (as Lightning's validation loop does): net.train(was) would
        # put a backbone the user keeps in eval mode (frozen BatchNorm) back into train mode
        modes = [(m, m.training) for m in self.net.modules()]
        self.net.eval()
        res = self.net(images)
        det = get_detections(FeatureShape(width=images.shape[3], height=images.shape[2]), res, self.anchor_info)
        out = non_max_suppression(det, self.val_nms_conf_threshold, self.val_nms_iou_threshold)
        for m, was in modes:
            m.training = was
        return targets, out

    # exp.py:164-185 + Lightning automatic optimisation
    def optimize(self, batch, num_training_batches: int):
        self.configure_optimizers()
        if self.ema is not None and self.ema.is_applied:
            raise RuntimeError("optimize() while ema.applied(): the step would train the averaged weights; leave the applied() "
                               "block first")
        self._num_training_batches = num_training_batches
        if self.graphed:
            return self._optimize_graphed(batch, num_training_batches)
        if self.multi_scale:
            batch = self._multi_scale_batch(batch)
        if self._window.first:                 # (a window's later micro-batches accumulate into .grad, Engine._publish_grads)
            self.optimizer.zero_grad(set_to_none=True)
        total = self.training_step(batch)
        total.backward()
        if self._window.advance():
            self._optimizer_step(num_training_batches)
        return total

    def step_accumulated(self):
        """Close an open accumulation window now (Lightning's is_final_batch rule: the last batch of an epoch steps the optimizer
        on what has been accumulated, its micro-batches keeping the B / N scale).  fit_epoch calls it; it does nothing when no
        window is open.  Returns whether an optimizer step ran."""
        if self.optimizer is None:
            return False
        n = self._num_training_batches
        if self.graphed:
            if self._gstep is None or self.accumulate_grad_batches == 1:
                return False
            eng = self.net.engine()
            if eng.accumulation is None or not eng.accumulation.flush_needed:
                return False
            self._warmup(n)
            if isinstance(self.optimizer, FusedAdam):
                self._gstep.flush(grad_scale=1.0 / self.optimizer.world_size, gradient_clip_val=self.optimizer.gradient_clip_val,
                                  adam=self.optimizer.hyper())
            else:
                lr, mom, wd = self.optimizer.hyper()
                self._gstep.flush(lr, mom, wd, 1.0 / self.optimizer.world_size, gradient_clip_val=self.optimizer.gradient_clip_val)
            self._graphed_stepped()
            return True
        if not self._window.flush_needed:
            return False
        self._window.reset()
        self._optimizer_step(n)
        return True

    def _optimizer_step(self, num_training_batches: int):
        """the eager route's per-window work: warm-up hook, clipping, optimizer.step(), EMA, global_step"""
        self._warmup(num_training_batches)
        if self._clipping():
            if isinstance(self.optimizer, (FusedSGD, FusedAdam)):
                # clipping is inside FusedSGD.step() / FusedAdam.step(); the norm stays a device scalar until the metrics are fetched
                self.optimizer.step()
                self.logged["grad_norm"] = self.net.engine().clip[0].clone()
            else:          # a torch network / optimizer: what Lightning's own hook does between backward and step
                params = [p for g in self.optimizer.param_groups for p in g["params"]]
                if self.gradient_clip_algorithm == "norm":
                    self.logged["grad_norm"] = torch.nn.utils.clip_grad_norm_(params, self.gradient_clip_val).detach()
                else:
                    self.logged["grad_norm"] = torch.linalg.vector_norm(
                        torch.stack([torch.linalg.vector_norm(p.grad) for p in params if p.grad is not None])).detach()
                    torch.nn.utils.clip_grad_value_(params, self.gradient_clip_val)
                self.optimizer.step()
        else:
            self.optimizer.step()
        if self.ema is not None:
            self.ema.update()
        self.global_step += 1

    # ------------------------------------------------------------------ weight EMA
    def ema_state_dict(self) -> Optional[dict]:
        """the EMA's state (save_checkpoint(ema_state=...)); None without ema=True"""
        if self.ema is not None:
            return self.ema.ema_state_dict()
        if self._ema_pending is not None:
            return dict(self._ema_pending)
        if not self._ema_on:
            return None
        self.configure_optimizers()
        return self.ema.ema_state_dict()

    def load_ema_state_dict(self, state: dict):
        if not self._ema_on:
            raise RuntimeError("load_ema_state_dict: the experiment was built without ema=True")
        if self.ema is not None:
            self.ema.load_ema_state_dict(state)
        else:
            self._ema_pending = dict(state)

    # ------------------------------------------------------------------ multi-scale
    def _multi_scale_holder(self):
        return self._gstep if (self.graphed and self._gstep is not None) else self._ms_schedule

    def multi_scale_state_dict(self) -> dict:
        """the size schedule's state (save_checkpoint(multi_scale_state=...))"""
        h = self._multi_scale_holder()
        if h is not None:
            return h.state_dict()
        return dict(self._ms_pending) if self._ms_pending is not None else {"seed": self.multi_scale_seed, "draws": 0, "steps": 0}

    def load_multi_scale_state_dict(self, state: dict):
        h = self._multi_scale_holder()
        if h is not None:
            h.load_state_dict(state)
        else:
            self._ms_pending = dict(state)

    def _multi_scale_batch(self, batch):
        """the eager route: the batch resized by kodhip_multiscale_batch to the drawn size (fp32 NCHW for the module's
        forward) and its boxes, scaled by the same launch, as BatchedTargets"""
        from ....core.label_assignment.yv5 import BatchedTargets
        from ....engine.multiscale import MultiScaleSchedule, resize_batch
        images, targets, rest = batch
        B, _, H, W = images.shape
        eng = self.net.engine()
        if self._ms_schedule is None:
            self._ms_schedule = MultiScaleSchedule(H, W, self.multi_scale_seed, self.multi_scale_range,
                                                   max(b.stride for b in eng.g.bufs), self.multi_scale_interval)
            if self._ms_pending is not None:
                self._ms_schedule.load_state_dict(self._ms_pending)
                self._ms_pending = None
        h, w = self._ms_schedule.next()
        x = (images if images.dtype == torch.float32 else images.float()).contiguous()
        bt = targets if isinstance(targets, BatchedTargets) else BatchedTargets.from_targets(targets, x.device)
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=x.device)
        pairs = self._ms_pairs.get((B, h, w))
        if pairs is None:
            pairs = self._ms_pairs[(B, h, w)] = torch.empty((B, h, w // 2, 8), dtype=torch.bfloat16, device=x.device)
        boxes = torch.empty_like(bt.boxes)
        resize_batch(eng.lib, x, pairs, h, w, out_f32=out, boxes_in=bt.boxes, boxes_out=boxes, n=bt.n)
        return out, BatchedTargets(boxes, bt.labels, bt.samples, bt.n), rest

    def _warmup(self, num_training_batches: int):
        if self.optimizer_warmup_updater is not None:
            nw = max(round(num_training_batches * self.optimizer_warmup_updater.warmup_epochs), 100)
            if self.global_step <= nw:
                self.optimizer_warmup_updater(current_step=self.global_step, current_epoch=self.current_epoch,
                                              max_warmup_steps=nw, sch_fn=self.sch_fn, optimizer=self.optimizer)

    def _graphed_optimizer(self) -> str:
        """which fused update the captured step ends with (GraphedTrainStep(optimizer=...))"""
        if isinstance(self.optimizer, FusedAdam):
            return "adam"
        if isinstance(self.optimizer, FusedSGD):
            return "sgd"
        raise RuntimeError(f"graphed=True needs the HIP network's FusedSGD or FusedAdam (torch.optim.SGD / Adam / AdamW through "
                           f"SmartOptimizer), not {type(self.optimizer).__name__}")

    def _optimize_graphed(self, batch, num_training_batches: int):
        from ....engine.graphed import GraphedTrainStep
        images, targets, _ = batch
        if self._gstep is None and self.multi_scale:
            from ....engine.multiscale import MultiScaleTrainStep
            B, _, H, W = images.shape
            opt = self.optimizer
            self._gstep = MultiScaleTrainStep(self.net, self.loss, B, H, W, self.max_targets,
                                              gradient_clip_val=opt.gradient_clip_val,
                                              gradient_clip_algorithm=opt.gradient_clip_algorithm,
                                              skip_nonfinite=opt.skip_nonfinite, track_grad_norm=opt.track_grad_norm,
                                              scale_range=self.multi_scale_range, interval=self.multi_scale_interval,
                                              seed=self.multi_scale_seed, max_graphs=self.multi_scale_max_graphs,
                                              optimizer=self._graphed_optimizer(),
                                              accumulate_grad_batches=self.accumulate_grad_batches)
            if self._ms_pending is not None:
                self._gstep.load_state_dict(self._ms_pending)
                self._ms_pending = None
        if self._gstep is None:
            B, _, H, W = images.shape
            opt = self.optimizer
            self._gstep = GraphedTrainStep(self.net, self.loss, B, H, W, self.max_targets,
                                           gradient_clip_val=opt.gradient_clip_val,
                                           gradient_clip_algorithm=opt.gradient_clip_algorithm,
                                           skip_nonfinite=opt.skip_nonfinite,
                                           track_grad_norm=opt.track_grad_norm,
                                           optimizer=self._graphed_optimizer(),
                                           accumulate_grad_batches=self.accumulate_grad_batches).capture(images, targets)
        self._warmup(num_training_batches)
        if isinstance(self.optimizer, FusedAdam):
            total, (box, obj, cls) = self._gstep(images, targets, grad_scale=1.0 / self.optimizer.world_size,
                                                 gradient_clip_val=self.optimizer.gradient_clip_val, adam=self.optimizer.hyper())
        else:
            lr, mom, wd = self.optimizer.hyper()
            total, (box, obj, cls) = self._gstep(images, targets, lr, mom, wd, 1.0 / self.optimizer.world_size,
                                                 gradient_clip_val=self.optimizer.gradient_clip_val)
        self.logged = {"obj": obj, "cls": cls, "box": box}
        if self._clipping():
            self.logged["grad_norm"] = self._gstep.grad_norm[0]          # (static, like the loss parts: the last update's norm)
        if self._gstep.stepped:               # (accumulate_grad_batches > 1: only the call that closed a window)
            self._graphed_stepped()
        return total.clone()

    def _graphed_stepped(self):
        """what follows an optimizer update of the graphed route (every call, or the one that closed an accumulation window)"""
        if self.ema is not None:              # behind the replay, on the same stream, outside the captured graph
            self.ema.update()
        self.optimizer.steps_taken += 1
        # the replayed graph contains the optimizer update: tell torch's bookkeeping that a step happened (LambdaLR.step() checks
        # optimizer._step_count to warn about a scheduler stepped before the optimizer)
        self.optimizer._step_count = getattr(self.optimizer, "_step_count", 0) + 1
        self.global_step += 1

    def end_epoch(self):
        """Lightning steps the epoch-interval scheduler: LambdaLR sets lr = initial_lr * lr_lambda(epoch)."""
        self.configure_optimizers()
        self.current_epoch += 1
        self.scheduler.step()

    def fit_epoch(self, batches: Sequence, num_training_batches: Optional[int] = None):
        n = num_training_batches or len(batches)
        _lib.limit_host_threads()      # the epoch loops are the library's own: size torch's host pool to the cgroup share
        with _gc_paused():
            losses = [self.optimize(b, n).detach() for b in batches]
            self.step_accumulated()        # the epoch's last batch closes a partial accumulation window
        self.end_epoch()
        return torch.stack(losses)

    def validate(self, batches: Sequence, num_classes: int, class_names=None) -> dict:
        ev = DeviceMAPEvaluator(num_classes, class_names)
        cm = None
        if self.val_confusion:
            from ...callbacks.confusion import DeviceConfusionMatrix
            cm = self.confusion = DeviceConfusionMatrix(num_classes, class_names, self.val_confusion_conf, self.val_confusion_iou)
        vm = None
        if self.val_metrics:
            from ...callbacks.val_metrics import DeviceDetectionMetrics
            vm = self.metrics = DeviceDetectionMetrics(num_classes, class_names)
        extra = [c for c in (cm, vm) if c is not None]
        _lib.limit_host_threads()
        if self.eval_fused is not None:
            self.net.fuse_eval(self.eval_fused)
        if self._ema_on:
            self.configure_optimizers()
        # ema=True: the averaged weights are in the network while the batches run (train.py validates ema.ema)
        with _gc_paused(), (self.ema.applied() if self.ema is not None else contextlib.nullcontext()):
            for b in batches:
                targets, dets = self.validation_step(b)
                if extra:                  # every consumer takes the batch's boxes as one device upload
                    if not isinstance(targets, BatchedTargets):
                        targets = BatchedTargets.from_targets(targets, dets[0].device if len(dets) else torch.device("cuda"))
                    ev.add_batch(targets, dets)
                    for c in extra:
                        c.add_batch(targets, dets)
                else:
                    ev.add_batch(targets, dets)
        pg = self._val_group()
        if pg is not None and self.val_process_group == "auto":
            self._all_ranks_validate(pg)
        report = ev.get_report(pg, self.val_sync)
        if cm is not None:
            pc = cm.per_class(pg)
            for c, name in enumerate(cm.names):
                report[f"precision_{name}"] = float(pc["precision"][c])
                report[f"recall_{name}"] = float(pc["recall"][c])
        if vm is not None:
            res = vm.compute(pg)
            report.update({"metrics/precision": res["mp"], "metrics/recall": res["mr"], "metrics/f1": res["mf1"],
                           "metrics/best_conf": res["best_conf"], "metrics/mAP_0.5": res["map50"],
                           "metrics/mAP_0.5:0.95": res["map"]})
        return report

    def _all_ranks_validate(self, pg, timeout_s: float = 300.0):
        """The default cross-rank report ("auto") is a collective: every rank of the data-parallel group must call
        validate().  A caller that validates on a subset of ranks (set val_process_group = None for that) would otherwise
        hang in the report's all-reduce with no message; where the group's backend can time a barrier (gloo) it is
        checked here first and the error says what to change."""
        import datetime
        import torch.distributed as dist
        if dist.get_backend(pg) != "gloo":
            return
        try:
            dist.monitored_barrier(pg, timeout=datetime.timedelta(seconds=timeout_s))
        except RuntimeError as e:
            raise RuntimeError("validate(): not every rank of the data-parallel group entered validation within "
                               f"{timeout_s:.0f} s. The default val_process_group='auto' averages the report over that group "
                               "(the reference's log_dict(sync_dist=True)); to validate on a subset of ranks set "
                               "experiment.val_process_group = None.") from e

    def _val_group(self):
        pg = self.val_process_group
        if isinstance(pg, str) and pg == "auto":
            eng = getattr(self.net, "_engine", None)
            if eng is None or getattr(eng, "world_size", 1) <= 1:
                return None
            import torch.distributed as dist
            return eng.process_group if eng.process_group is not None else dist.group.WORLD
        return pg
