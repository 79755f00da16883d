"""Launch trace of one eager training step: every libkodhip call, every stream / event operation and every aten operation
torch issues inside the step, one line each in issue order, with nothing process-dependent in the text.  The eager sequence of
stream operations is what a capture turns into graph nodes and edges, so equal traces mean an equal captured graph
(tests/test_hip_launch_trace.py pins the traces of CONFIGS against tests/golden/launch_trace.json).

The recorded step is the third - after two warm-up steps on a side stream, as GraphedTrainStep.capture runs them:
net.train_step(...), eng.wait_grads(), eng.sgd_step_device().  Streams are written as roles (main, wg, head, br, aux, then
s<n> by first appearance), events as e<n> by first record, pointers as <engine object>+<byte offset> (tensors the step itself
allocates: t<n> by allocation order).  A non-null pointer that resolves to nothing is an error.  Nothing is synchronised or
timed inside the step: the recording does not change what it records.

The eval_forward* configurations record one eval forward (net.eval(), net(x) under torch.no_grad()) the same way.

A second mode keeps what the launch text does not show: the (family, algorithmic bytes, name) sequence of eng.profile - the
numbers bench.py --full builds its roofline table from, and the one-stream schedule of a profiled step - for the cases of
PROFILE_CASES (tests/golden/profile_families.json).

usage (GPU box):  python tools/launch_trace.py CONFIG [--out FILE]      one configuration's trace (a fresh process each:
                                                                       the engine reads its switches once)
                  python tools/launch_trace.py --list
                  python tools/launch_trace.py --record FILE [--keep DIR]   every configuration in a child process -> golden JSON
                  python tools/launch_trace.py --profile CASE [--out FILE]  one case's eng.profile sequence as JSON
                  python tools/launch_trace.py --record-profile FILE        every case in a child process -> golden JSON
"""
import bisect
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, B, S, SEED = 10, 2, 160, 2023                  # yv5s as in tests/test_hip_freeze.py
CHILD_TIMEOUT = 240

_BB = lambda n: n.startswith("backbone.")
_FREEZE = {
    "backbone": _BB,
    "neck": lambda n: n.startswith("neck."),
    "stem": lambda n: n.startswith("backbone.stem."),
    "mid_conv_weight": lambda n: n == "backbone.stages.stage2.blocks.1.blocks.0.conv1.0.weight",
    "bn_affine": lambda n: n in ("neck.reduce_layers.2.1.weight", "neck.reduce_layers.2.1.bias"),
    "head_cls": lambda n: n == "ml_head.cls_head.conv.weight",
    "backbone_affine": lambda n: _BB(n) and (n.endswith(".1.weight") or n.endswith(".1.bias")),
}


def _cfg(env=None, model="net", freeze=None, bn_eval=None, dist=None, clip=None, eval_forward=False):
    """env: engine switches; model: net | csp | csp_relu; freeze: key of _FREEZE; bn_eval: backbone | short | all;
    dist: None or (sync_batchnorm,) on a 1-rank group; clip: (algorithm, value, skip_nonfinite, track_grad_norm);
    eval_forward: the step is one eval forward of the whole network instead of a training step"""
    return dict(env=env or {}, model=model, freeze=freeze, bn_eval=bn_eval, dist=dist, clip=clip, eval_forward=eval_forward)


_COLL = {"KODHIP_FORCE_COLLECTIVES": "1"}
CONFIGS = {
    "default": _cfg(),
    "sw_wgrad_overlap0": _cfg({"KODHIP_WGRAD_OVERLAP": "0"}),
    "sw_branch_overlap0": _cfg({"KODHIP_BRANCH_OVERLAP": "0"}),
    "sw_no_dual": _cfg({"KODHIP_NO_DUAL": "1"}),
    "sw_no_dual_wgrad": _cfg({"KODHIP_NO_DUAL_WGRAD": "1"}),
    "sw_no_bnred": _cfg({"KODHIP_NO_BNRED": "1"}),
    "sw_dx_fp32": _cfg({"KODHIP_DX_FP32": "1"}),
    "sw_stem_bwd_fused0": _cfg({"KODHIP_STEM_BWD_FUSED": "0"}),
    "sw_stem_bwd_stream_wg": _cfg({"KODHIP_STEM_BWD_STREAM": "wg"}),
    "fz_backbone": _cfg(freeze="backbone"),
    "fz_stem": _cfg(freeze="stem"),
    "fz_mid_conv_weight": _cfg(freeze="mid_conv_weight"),
    "fz_bn_affine": _cfg(freeze="bn_affine"),
    "fz_head_cls": _cfg(freeze="head_cls"),
    "fz_backbone_dx_fp32": _cfg({"KODHIP_DX_FP32": "1"}, freeze="backbone"),
    "fz_neck_dx_fp32": _cfg({"KODHIP_DX_FP32": "1"}, freeze="neck"),
    "bn_backbone_eval": _cfg(bn_eval="backbone"),
    "bn_backbone_eval_frozen_affine": _cfg(bn_eval="backbone", freeze="backbone_affine"),
    "bn_short_conv_eval": _cfg(bn_eval="short"),
    "fz_bn_backbone_no_dual": _cfg({"KODHIP_NO_DUAL": "1"}, freeze="backbone", bn_eval="backbone"),
    "act_relu": _cfg(model="csp_relu", bn_eval="all"),
    "sub_csp": _cfg(model="csp"),
    "sub_csp_short_eval": _cfg(model="csp", bn_eval="short"),
    "coll_buckets": _cfg(_COLL, dist=(False,)),
    "coll_syncbn_rccl": _cfg({**_COLL, "KODHIP_SYNCBN": "rccl"}, dist=(True,)),
    "coll_syncbn_peer": _cfg({**_COLL, "KODHIP_SYNCBN": "peer"}, dist=(True,)),
    "coll_inorder": _cfg({**_COLL, "KODHIP_SYNCBN": "rccl", "KODHIP_COMM_OVERLAP": "0"}, dist=(True,)),
    "coll_fz_backbone": _cfg(_COLL, freeze="backbone", dist=(False,)),
    "coll_clip_norm": _cfg(_COLL, dist=(False,), clip=("norm", 1.0, False, False)),
    "clip_norm": _cfg(clip=("norm", 1.0, False, False)),
    "clip_value": _cfg(clip=("value", 0.01, False, False)),
    "clip_skip_nonfinite": _cfg(clip=(None, None, True, False)),
    "clip_track_grad_norm": _cfg(clip=(None, None, False, True)),
    "eval_forward": _cfg(eval_forward=True),
    "eval_forward_fused": _cfg({"KODHIP_EVAL_FUSED": "1"}, eval_forward=True),
}
# eng.profile cases (tests/golden/profile_families.json): case -> the configuration whose step is profiled
PROFILE_CASES = {"train_step": "default", "eval_forward": "eval_forward", "eval_forward_fused": "eval_forward_fused"}
SWITCHES = sorted({k for c in CONFIGS.values() for k in c["env"]})


# ---------------------------------------------------------------------------------------------- the recorder
class Trace:
    """The recorder: stands in for the ctypes handle (attribute access gives a recording wrapper of the real entry point)
    and receives the stream / event / aten operations from the patches below.  Records only while `active`."""

    def __init__(self, real, signatures):
        self._real, self._sig = real, signatures
        self._fns = {}
        self.active = False
        self.lines = []
        self.launches = {}
        self.streams, self.events, self._keep = {}, {}, []
        self._bases, self._ranges, self._seen = [], [], set()      # engine objects: sorted base addresses, (base, size, name)
        self._exact = {}                                           # opaque handles: address -> name
        self._temps, self._temp_ids = [], {}                       # tensors the step allocates: (base, size, name), newest last
        self._depth = 0

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._real, name)

            def fn(*args, _real=real, _name=name):
                if self.active:
                    self._lib_call(_name, args)
                return _real(*args)
            self._fns[name] = fn
        return fn

    # -- names
    def add_range(self, base, size, name):
        if base and size and base not in self._seen:
            self._seen.add(base)
            i = bisect.bisect(self._bases, base)
            self._bases.insert(i, base)
            self._ranges.insert(i, (base, size, name))

    def add_tensor(self, t, name, temp=False):
        st = t.untyped_storage()
        base, size = st.data_ptr(), st.nbytes()
        if not base or not size:
            return
        if not temp:
            self.add_range(base, size, name)
        elif self._find(base, self._bases, self._ranges) is None and st._cdata not in self._temp_ids:
            # the storage is kept alive with the trace: no block is handed out twice, so a name means one allocation
            self._temp_ids[st._cdata] = st
            self._temps.append((base, size, "t%d" % len(self._temps)))

    @staticmethod
    def _find(p, bases, ranges):
        i = bisect.bisect_right(bases, p) - 1
        if i >= 0:
            base, size, name = ranges[i]
            if p < base + size:
                return "%s+%d" % (name, p - base)
        return None

    def ptr(self, p, what):
        if p is None:
            return "null"
        if isinstance(p, C.c_void_p):
            p = p.value
        if not p:
            return "null"
        if p in self._exact:
            return self._exact[p]
        r = self._find(p, self._bases, self._ranges)
        if r is not None:
            return r
        for base, size, name in reversed(self._temps):
            if base <= p < base + size:
                return "%s+%d" % (name, p - base)
        raise RuntimeError("launch trace: pointer %#x of %s resolves to no engine object" % (p, what))

    def stream(self, sid):
        if isinstance(sid, C.c_void_p):
            sid = sid.value
        sid = sid or 0
        if sid not in self.streams:
            self.streams[sid] = "s%d" % sum(1 for v in self.streams.values() if v[0] == "s" and v[1:].isdigit())
        return self.streams[sid]

    def event(self, ev, new=False):
        k = id(ev)
        if k not in self.events:
            if not new:
                return "e?"              # (waited for, never recorded inside the step)
            self.events[k] = "e%d" % len(self.events)
            self._keep.append(ev)        # ids stay unique while the trace lives
        return self.events[k]

    # -- lines
    def _struct(self, s, what):
        out = []
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            if ftype is C.c_void_p:
                out.append("%s=%s" % (fname, self.ptr(v, what + "." + fname)))
            elif isinstance(v, C.Array):
                out.append("%s=%s" % (fname, [x for x in v]))
            else:
                out.append("%s=%r" % (fname, v))
        return "{" + " ".join(out) + "}"

    def _lib_call(self, name, args):
        types = self._sig[name][1]
        assert len(types) == len(args), (name, len(types), len(args))
        out = []
        for i, (a, t) in enumerate(zip(args, types)):
            what = "%s arg %d" % (name, i)
            if isinstance(a, C.Array) and issubclass(a._type_, C.Structure):
                out.append("[" + " ".join(self._struct(s, what) for s in a) + "]")
            elif t is C.c_void_p:
                v = a.value if isinstance(a, C.c_void_p) else a
                if i == len(args) - 1 and (not v or v in self.streams):
                    out.append("@" + self.stream(v))
                else:
                    try:
                        out.append(self.ptr(v, what))
                    except RuntimeError:
                        if i != len(args) - 1:
                            raise
                        out.append("@" + self.stream(v))           # a stream first seen here
            elif isinstance(a, (int, float, bytes)) or a is None:
                out.append(repr(a))
            else:
                out.append("&" + type(a).__name__)                 # (an out-parameter passed by reference)
        self.launches[name] = self.launches.get(name, 0) + 1
        self.lines.append("lib %s(%s)" % (name, ", ".join(out)))

    def sync_op(self, text):
        self.lines.append(text)

    def aten(self, func, args, kwargs, cur):
        import torch
        descs = []

        def walk(o):
            if isinstance(o, torch.Tensor):
                d = "%s%s" % (str(o.dtype).replace("torch.", ""), list(o.shape))
                if o.is_cuda:
                    try:
                        d += ":" + self.ptr(o.data_ptr(), str(func)) if o.numel() else ":empty"
                    except RuntimeError:
                        d += ":?"
                else:
                    d += ":host"
                descs.append(d)
            elif isinstance(o, (list, tuple)):
                if o and all(type(x) is int for x in o):
                    descs.append(str(list(o)))          # (a factory's size argument)
                for x in o:
                    walk(x)
        for a in args:
            walk(a)
        walk(list((kwargs or {}).values()))
        self.lines.append("aten %s(%s) @%s" % (func, ", ".join(descs), self.stream(cur)))

    def text(self):
        return "\n".join(self.lines) + "\n"


def _walk(tr, obj, name, depth=0, seen=None):
    """register every tensor / ctypes table reachable from `obj` under its attribute path (first name of a storage wins)"""
    import torch
    seen = set() if seen is None else seen
    if obj is None or isinstance(obj, (str, bytes, int, float, bool)) or id(obj) in seen or depth > 6:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        tr.add_tensor(obj, name)
        if isinstance(obj, torch.nn.Parameter) and obj.grad is not None:
            tr.add_tensor(obj.grad, name + ".grad")
    elif isinstance(obj, C.c_void_p):
        if obj.value:
            tr._exact[obj.value] = name
    elif isinstance(obj, (C.Array, C.Structure)):
        tr.add_range(C.addressof(obj), C.sizeof(obj), name)
    elif isinstance(obj, dict):
        for i, (k, v) in enumerate(obj.items()):
            _walk(tr, v, "%s[%s]" % (name, k if isinstance(k, str) else "#%d" % i), depth + 1, seen)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _walk(tr, v, "%s[%d]" % (name, i), depth + 1, seen)
    elif type(obj).__module__.startswith("object_detection_cib_amd") or isinstance(obj, torch.nn.Module):
        if isinstance(obj, torch.nn.Module):
            for k, v in list(obj.named_parameters(recurse=False)) + list(obj.named_buffers(recurse=False)):
                _walk(tr, v, name + "." + k, depth + 1, seen)
        attrs = list(getattr(obj, "__dict__", {}).items())
        for cls in type(obj).__mro__:
            attrs += [(k, getattr(obj, k)) for k in getattr(cls, "__slots__", ()) if hasattr(obj, k)]
        for k, v in attrs:
            if k not in ("_modules", "_parameters", "_buffers", "lib", "g", "opt"):
                _walk(tr, v, name + "." + k, depth + 1, seen)


def _register(tr, eng, extra):
    # the engine's own tensors first, so that views (parameters, gradients, per-unit slices) resolve to the arenas
    # (the current buffer set under the names the golden file was recorded with: the engine once kept these on itself,
    # the per-unit records as `ustate`, the per-head ones as dicts `hstate`)
    bs = eng.cur
    named = dict(wg_part=bs.wg_part, stem_part=bs.stem_part, act=bs.act, gact=bs.gact, gact32=bs.gact32, ustate=bs.units,
                 hstate={n: dict(dy=hs.dy, ws=hs.ws) for n, hs in bs.heads.items()}, pool_idx=bs.pool_idx)
    for k in ("p_arena", "g_arena", "m_arena", "rm_arena", "rv_arena", "nbt_arena", "gid", "fpack", "dpack", "wg_part",
              "stem_part", "act", "gact", "gact32", "ustate", "hstate", "pool_idx", "clip", "norm_ws", "hyper", "keep_mask"):
        if k in named or hasattr(eng, k):
            _walk(tr, named[k] if k in named else getattr(eng, k), k)
    _walk(tr, eng, "eng")
    for name, obj in extra.items():
        _walk(tr, obj() if callable(obj) else obj, name)


def _patch(tr):
    """route torch's stream / event operations and aten dispatches into the trace (outermost call only: Stream.wait_stream
    is built from record_event + wait_event)"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    cur = lambda: torch.cuda.current_stream().cuda_stream

    def wrap(cls, meth, describe):
        orig = getattr(cls, meth)

        def patched(self, *a, **k):
            if tr.active and tr._depth == 0:
                tr.sync_op(describe(self, *a, **k))
            tr._depth += 1
            try:
                return orig(self, *a, **k)
            finally:
                tr._depth -= 1
        setattr(cls, meth, patched)

    sname = lambda s: tr.stream(s.cuda_stream if s is not None else cur())
    wrap(torch.cuda.Event, "record", lambda ev, stream=None: "event %s record @%s" % (tr.event(ev, True), sname(stream)))
    wrap(torch.cuda.Event, "wait", lambda ev, stream=None: "event %s wait @%s" % (tr.event(ev), sname(stream)))
    wrap(torch.cuda.Stream, "wait_event", lambda s, ev: "stream %s wait_event %s" % (sname(s), tr.event(ev)))
    wrap(torch.cuda.Stream, "wait_stream", lambda s, other: "stream %s wait_stream %s" % (sname(s), sname(other)))
    wrap(torch.cuda.Stream, "record_event",
         lambda s, event=None: "stream %s record_event %s" % (sname(s), tr.event(event, True) if event is not None else "new"))

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if tr.active:
                tr.aten(func, args, kwargs, cur())
            out = func(*args, **(kwargs or {}))
            if tr.active:
                for o in (out if isinstance(out, (list, tuple)) else (out,)):
                    if isinstance(o, torch.Tensor) and o.is_cuda:
                        tr.add_tensor(o, None, temp=True)
            return out
    return Mode


# ---------------------------------------------------------------------------------------------- one configuration
def _set_modes(cfg, net):
    import torch
    BN = torch.nn.BatchNorm2d
    net.train()
    ev = cfg["bn_eval"]
    if ev == "backbone":
        net.backbone.eval()
    elif ev == "all":
        for m in net.modules():
            if isinstance(m, BN):
                m.eval()
    elif ev == "short":
        if hasattr(net, "short_conv"):
            net.short_conv.eval()
        else:
            name = next(u.name for u in net.graph.units if u.name.endswith(".short_conv"))
            net.get_submodule(name).eval()
    if cfg["freeze"]:
        pick = _FREEZE[cfg["freeze"]]
        for n, p in net.named_parameters():
            p.requires_grad_(not pick(n))


def _enter_config(name):
    """this process takes the environment switches of configuration `name` (before the engine is built)"""
    cfg = CONFIGS[name]
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.pop("KODHIP_DEBUG_STAMPS", None)
    os.environ.update(cfg["env"])
    sys.path.insert(0, ROOT)
    return cfg


def profile_case(case):
    """-> [[family, algorithmic bytes, name], ...] of eng.profile over the third step of PROFILE_CASES[case]: the step runs
    eagerly with eng.profile = [] (every launch event-timed on one stream, no side branches)"""
    cfg = _enter_config(PROFILE_CASES[case])
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    step, eng, _ = _build_step(cfg, dev)
    for _ in range(2):
        step()
    eng.profile = []
    step()
    torch.cuda.synchronize()
    prof, eng.profile = eng.profile, None
    return [[fam, float(nb), name] for fam, _, _, nb, name in prof]


def trace_config(name):
    """-> Trace of configuration `name` (this process: environment switches are set here, before the engine is built)"""
    cfg = _enter_config(name)
    import torch
    from object_detection_cib_amd import _lib
    tr = Trace(_lib.lib(), _lib.SIGNATURES)
    _lib._lib = tr                                     # before the engine is built: engine/comm.py, engine/ddp.py see it too
    Mode = _patch(tr)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if cfg["dist"] is not None:
        import socket
        import torch.distributed as dist
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
    eng = None
    try:
        step, eng, extra = _build_step(cfg, dev)
        assert eng.lib is tr and eng.profile is None and not eng.stamps_on
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
            tr.streams[side.cuda_stream] = "main"
            for role in ("wg", "head", "br", "aux"):
                s = getattr(eng, role + "_stream")
                if s is not None and s.cuda_stream not in tr.streams:
                    tr.streams[s.cuda_stream] = role
            _register(tr, eng, extra)
            with Mode():
                tr.active = True
                try:
                    step()
                finally:
                    tr.active = False
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    finally:
        if cfg["dist"] is not None:
            import torch.distributed as dist
            torch.cuda.synchronize()
            for c in ((eng.comm, eng.comm_buckets, eng.peer) if eng is not None else ()):
                if c is not None:
                    c.close()
            dist.destroy_process_group()
    return tr


def _build_step(cfg, dev):
    import torch
    from oracle import synth
    hyper = ((0.02, 0.02, 0.02), (0.9,) * 3, (0.0, 5e-4, 0.0))
    if cfg["model"] != "net":
        from object_detection_cib_amd.nn.layers.csp import CSPLayer
        from object_detection_cib_amd.nn.networks.yolov5 import Yolov5BatchNorm2d
        torch.manual_seed(4)
        act = torch.nn.ReLU if cfg["model"] == "csp_relu" else torch.nn.SiLU
        net = CSPLayer(64, 128, 0.5, True, 2, Yolov5BatchNorm2d, act).to(dev)
        _set_modes(cfg, net)
        x = torch.randn(4, 64, 24, 40, generator=torch.Generator().manual_seed(1)).to(dev)
        w = torch.randn(4, 128, 24, 40, generator=torch.Generator().manual_seed(7)).to(dev)
        eng = net.engine()
        eng.set_hyper(*hyper)
        params = list(net.parameters())

        def step():
            for p in params:
                p.grad = None
            with torch.no_grad():
                eng.sync_freeze()
                eng.forward([x], training=True)
                eng.backward([], [w])          # Graph.inputs / outputs path: out_grads in, input gradients out
            eng.wait_grads()
            eng.sgd_step_device()
        return step, eng, dict(x=x, out_grad=w)
    from object_detection_cib_amd.core.types import FeatureShape
    from object_detection_cib_amd.core.anchors.info import voc_anchor_info
    from object_detection_cib_amd.core.bbox.iou import IoUCalculator
    from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo, BatchedTargets
    from object_detection_cib_amd.data.detection import DetectionTarget
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(SEED)
    net = Yolov5Network(3, NC, widen_factor=0.5, deepen_factor=0.33).to(dev)
    _set_modes(cfg, net)
    xs, tg = synth.batch(B, S, NC, SEED)
    asg = Yolov5LabelAssigner(AssignmentAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32)), 4.0)
    loss = Yolov5Loss(asg, Yolov5LossParams.get_default(), IoUCalculator("ciou", 1e-7), None)
    x = xs.to(dev)
    targets = BatchedTargets.from_targets(tuple(DetectionTarget(b, l) for b, l in tg), dev)
    eng = net.engine()
    if cfg["dist"] is not None:
        net.configure_distributed(None, sync_batchnorm=cfg["dist"][0], bucket_mb=0.5, native_rccl=True)
        assert eng.collectives and eng.comm is not None
    if cfg["eval_forward"]:
        net.eval()

        def step():
            with torch.no_grad():
                net(x)
        return step, eng, dict(x=x)
    eng.set_hyper(*hyper)
    if cfg["clip"] is not None:
        algo, val, skip, track = cfg["clip"]
        eng.configure_clip(algo, skip, track)
        eng.set_clip(val)
    shape = FeatureShape(width=S, height=S)
    params = list(net.parameters())

    def step():
        for p in params:
            p.grad = None
        net.train_step(x, loss, shape, targets, float(B))
        eng.wait_grads()
        eng.sgd_step_device()
    # (of the loss only what outlives a step: its results of the last step die inside the next one)
    return step, eng, dict(x=x, targets=targets, upstream=lambda: loss.__dict__.get("_upstream_cache"), pos_weight=loss.weights)


# ---------------------------------------------------------------------------------------------- children, golden file
def summary(text, launches=None):
    """what the golden file keeps of one trace"""
    lines = text.splitlines()
    if launches is None:
        launches = {}
        for ln in lines:
            if ln.startswith("lib "):
                k = ln[4:ln.index("(")]
                launches[k] = launches.get(k, 0) + 1
    return dict(lines=len(lines), launches=dict(sorted(launches.items())), sha256=hashlib.sha256(text.encode()).hexdigest())


def run_child(name, out_path, timeout=CHILD_TIMEOUT, profile=False):
    """One configuration (profile: one case of PROFILE_CASES) in a fresh process under its own time limit -> (return code,
    stderr tail).  A negative return code is a signal (an abort, a fault); None the time limit: start nothing more on the
    GPU after either."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + (["--profile"] if profile else []) +
                           [name, "--out", out_path], capture_output=True,
                           text=True, timeout=timeout, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        return None, str(e)
    return r.returncode, r.stderr[-3000:]


def record(path, keep=None):
    """keep: a directory that receives the traces themselves (to diff a later tree against)"""
    golden, failed = {}, []
    for name in CONFIGS:
        tmp = os.path.join(keep, name + ".trace") if keep else path + "." + name + ".trace"
        rc, err = run_child(name, tmp)
        if rc is None or rc < 0 or rc in (124, 134, 137, 139):
            sys.exit("launch trace of %s ended by a signal or its time limit (rc %s); nothing further was started\n%s" % (name, rc, err))
        if rc != 0:                      # (an ordinary Python error: the GPU is fine)
            failed.append(name)
            print(name, "FAILED rc", rc, err[-1500:], flush=True)
            continue
        golden[name] = summary(open(tmp).read())
        if not keep:
            os.remove(tmp)
        print(name, golden[name]["lines"], golden[name]["sha256"][:12], flush=True)
    with open(path, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    if failed:
        sys.exit("no trace of: " + " ".join(failed))


def record_profile(path):
    golden = {}
    for case in PROFILE_CASES:
        tmp = path + "." + case + ".tmp"
        rc, err = run_child(case, tmp, profile=True)
        if rc != 0:
            sys.exit("profile of %s: rc %s; nothing further was started\n%s" % (case, rc, err))
        golden[case] = json.load(open(tmp))
        os.remove(tmp)
        print(case, len(golden[case]), "launches", flush=True)
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n%s\n ]' % (case, ",\n".join("  " + json.dumps(r) for r in rows))
                                   for case, rows in sorted(golden.items())) + "\n}\n")


def main(argv):
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    if argv[0] == "--list":
        print("\n".join(CONFIGS))
        return 0
    if argv[0] == "--record":
        record(argv[1], argv[3] if len(argv) > 3 and argv[2] == "--keep" else None)
        return 0
    if argv[0] == "--record-profile":
        record_profile(argv[1])
        return 0
    if argv[0] == "--profile":
        text = json.dumps(profile_case(argv[1]))
        if len(argv) > 3 and argv[2] == "--out":
            with open(argv[3], "w") as f:
                f.write(text)
        else:
            print(text)
        return 0
    tr = trace_config(argv[0])
    if len(argv) > 2 and argv[1] == "--out":
        with open(argv[2], "w") as f:
            f.write(tr.text())
    else:
        sys.stdout.write(tr.text())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
