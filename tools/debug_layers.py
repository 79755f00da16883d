"""Per-layer activation comparison HIP vs fp32 oracle and vs bf16-emulated oracle (diagnostic)."""
import sys, torch
sys.path.insert(0, ".")
from oracle import synth, bf16_emul
from oracle.network import OracleYolov5
from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network

size = int(sys.argv[1]) if len(sys.argv) > 1 else 160
widen, deepen, nc, B, seed = 0.5, 0.33, 10, 2, 2023
def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
x, tg = synth.batch(B, size, nc, seed)
allacts = {}
for which in ("ref", "emu"):
    torch.manual_seed(seed); ref = OracleYolov5(3, nc, widen, deepen).train()
    acts = {}
    def hook(name, acts=acts):
        def f(m, i, o): acts[name] = o.detach().clone()
        return f
    if which == "emu":
        bf16_emul.emulate(ref)
    for name, m in ref.named_modules():
        if isinstance(m, torch.nn.Sequential) and len(m) == 3 and isinstance(m[0], torch.nn.Conv2d):
            m.register_forward_hook(hook(name))
            m[0].register_forward_hook(hook(name + ".raw"))
    ref(x)
    allacts[which] = acts
torch.manual_seed(seed); net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
outs = net.forward_raw(x.cuda())
eng = net.engine()
for u in eng.exec_units:
    st = eng.cur.units[u.name]
    raw = st.raw.float().permute(0, 3, 1, 2).cpu()
    a = eng.cur.act[u.dst.buf.name][..., u.dst.coff:u.dst.coff + u.dst.C].float().permute(0, 3, 1, 2).cpu()
    line = f"{u.name:52s}"
    for which in ("ref", "emu"):
        acts = allacts[which]
        line += f" {which}: raw={rel(raw, acts[u.name + '.raw']):.5f}"
        if u.residual is None:
            line += f" act={rel(a, acts[u.name]):.5f}"
        else:
            line += " act=  ---  "
    print(line)
