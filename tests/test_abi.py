"""CPU checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/kodhip.h
declares, and the ctypes table matches the header one to one (no compute calls: no GPU here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kodhip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kodhip_[a-z0-9_]+)\s*\(", src)))


def _params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % re.escape(name), src, flags=re.S)
    args = m.group(1).strip()
    return 0 if args in ("void", "") else len([a for a in args.split(",") if a.strip()])


@pytest.fixture(scope="module")
def built():
    from object_detection_cib_amd import build
    return build.build(verbose=False)


def test_header_symbols_exported(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built]).decode()
    exported = set(re.findall(r" T (kodhip_[a-z0-9_]+)", out))
    missing = [s for s in _declared() if s not in exported]
    assert not missing, missing


def test_ctypes_table_matches_header(built):
    from object_detection_cib_amd import _lib
    decl = set(_declared())
    table = set(_lib.SIGNATURES)
    assert table <= decl, sorted(table - decl)
    assert decl - table <= {"kodhip_set_error"}, sorted(decl - table)
    for name, (_, args) in _lib.SIGNATURES.items():
        assert len(args) == _params(name), (name, len(args), _params(name))


def test_library_loads_and_reports(built):
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 100
    assert h.kodhip_pack_desc_bytes() == 13 * 8
    assert h.kodhip_device_count() >= 0
    # argument validation happens before any launch, so it is testable without a GPU
    rc = h.kodhip_bn_silu_apply(None, 0, None, None, None, 0, 0, None, 0, 0, 0, 0, None)
    assert rc < 0 and b"bn_silu_apply" in h.kodhip_last_error()
    rc = h.kodhip_conv_fwd_raw(1, 1, 1, 1, 1, 8, 8, 12, 0, 12, 8, 1, 1, 1, 1, 0, 0, 32, 8, 0, None)
    assert rc < 0 and b"multiples of 8" in h.kodhip_last_error()


def test_plan_queries_launch_nothing(built):
    """kodhip_conv_plan_query / kodhip_conv_wgrad_plan_query answer from the geometry alone (no GPU, no pointer read):
    the dispatch rules they report are the ones tests/test_hip_conv_exact.py builds its cases on."""
    import ctypes as C
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    out = (C.c_int * 8)()

    def conv(op, B, Cin, H, W, N, k, s, p, Kp):
        assert h.kodhip_conv_plan_query(op, B, H, W, Cin, 0, Cin, N, k, k, s, s, p, p, Kp, N, 0, out) == 0, h.kodhip_last_error()
        return list(out)
    if any(os.environ.get(k) for k in ("KODHIP_ROW3", "KODHIP_NO_FAST", "KODHIP_FORCE_BN", "KODHIP_FORCE_BM", "KODHIP_S2_SEPARATE",
                                       "KODHIP_WGRAD_ROW3", "KODHIP_WGRAD_DMA", "KODHIP_WGRAD_SLOTS")):
        pytest.skip("a dispatch knob is set")
    # 256-pixel tiles: FAST, no ROW3, M >= 16384, K >= 512, N > 32
    assert conv(0, 1, 512, 128, 128, 64, 1, 1, 0, 512)[:4] == [256, 64, 0, 1]
    assert conv(0, 1, 512, 127, 128, 64, 1, 1, 0, 512)[0] == 128            # M = 16256
    assert conv(0, 1, 480, 128, 128, 64, 1, 1, 0, 480)[0] == 128            # K = 480
    assert conv(0, 1, 512, 128, 128, 32, 1, 1, 0, 512)[0] == 128            # N = 32
    assert conv(0, 5, 64, 60, 56, 160, 3, 1, 1, 576)[:3] == [128, 64, 1]    # 3x3 / stride 1: ROW3 keeps 128-pixel tiles
    # the parity classes of a stride-2 data gradient share one merged launch; the plain entry point leaves the FAST path
    assert conv(2, 4, 64, 128, 128, 128, 3, 2, 1, 0)[7] == 256 and conv(1, 4, 64, 128, 128, 128, 3, 2, 1, 9 * 128)[3] == 0
    assert conv(3, 2, 32, 16, 16, 64, 3, 2, 1, 0)[5] == 2                   # folded: 4 x Cin = 128 columns as two 64-column tiles
    # persistent blocks over several pixel tiles
    m = conv(0, 1, 32, 130, 128, 512, 3, 1, 1, 288)
    assert m[4] == 130 and m[6] == 96
    assert h.kodhip_conv_plan_query(9, 1, 8, 8, 32, 0, 32, 32, 1, 1, 1, 1, 0, 0, 32, 32, 0, out) < 0 and b"bad op" in h.kodhip_last_error()
    assert h.kodhip_conv_plan_query(0, 1, 8, 8, 32, 0, 32, 32, 1, 1, 1, 1, 0, 0, 32, 32, 0, None) < 0

    def wgrad(B, Cin, H, W, N, k, s, p, Kp, dual=0):
        assert h.kodhip_conv_wgrad_plan_query(B, H, W, Cin, Cin, N, k, k, s, s, p, p, Kp, N, dual, out) == 0, h.kodhip_last_error()
        return list(out)
    assert wgrad(2, 32, 20, 12, 32, 3, 1, 1, 288)[:6] == [32, 32, 1, 1, 1, 1]           # ROW3 where it measured faster: N <= 32
    assert wgrad(2, 64, 20, 12, 64, 3, 1, 1, 576)[:3] == [64, 128, 0]
    assert wgrad(2, 32, 20, 12, 32, 3, 2, 1, 288)[:3] == [32, 288, 0]                   # one block over all of K
    w = wgrad(2, 64, 70, 65, 32, 1, 1, 0, 64)
    assert w[:2] == [32, 64] and w[7] == 1 and w[6] == h.kodhip_conv_wgrad_splits_geo(2, 70, 65, 64, 64, 32, 1, 1, 1, 1, 0, 0, 64, 32)
    assert wgrad(2, 64, 70, 65, 32, 1, 1, 0, 64, dual=1)[6] == h.kodhip_conv_wgrad_dual_splits(2, 70, 65, 64, 64, 32, 64, 32)
    assert h.kodhip_conv_wgrad_plan_query(2, 70, 65, 64, 64, 32, 1, 1, 1, 1, 0, 0, 64, 32, 0, None) < 0


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    net = Yolov5Network(3, 10, widen_factor=0.25, deepen_factor=0.33)
    with pytest.raises(RuntimeError, match="MI355X|GPU|cuda"):
        net(torch.zeros(1, 3, 64, 64))


def test_pmc_evidence_matches_kernel_sources():
    """profiles/r06_pmc_traffic.json (what bench.py quotes as roofline.traffic) must have been collected on the kernel
    sources in the tree: a stale file fails HERE, loudly, instead of being quoted (bench.py itself then reports
    traffic null).  Fix: tools/collect_evidence.sh on the GPU box + tools/refresh_profiles.py, or delete the file."""
    import json
    import os
    from object_detection_cib_amd import build as kb
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r06_pmc_traffic.json")
    if not os.path.exists(p):
        pytest.skip("no PMC evidence committed")
    assert json.load(open(p))["csrc_digest"] == kb.source_digest(), "PMC evidence is older than csrc/: re-collect it"
